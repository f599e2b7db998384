// Host-side logic of the kernel launchers (csrc/*.hip), run under AddressSanitizer and
// UndefinedBehaviorSanitizer on the CPU: split-count planning, scratch sizing and the
// argument validation that must reject a bad call BEFORE anything is launched.  Built by
// tests/test_native_host_sanitizers.py with the sanitizers on the host side only
// (hipcc -Xarch_host -fsanitize=...); no kernel is launched, so no GPU is needed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launchers.h"

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

// ---------------------------------------------------------------- attention plans (csrc/attn_plan.h)
// The expectations below are written out from the launch tables the kernels were tuned with; they
// do not call the code under test.
using orion::AttnLaunch;

static bool is_launch(const AttnLaunch& l, int kernel, int grid, int block, int lds) {
  return l.kernel == kernel && l.grid == grid && l.block == block && l.lds == lds;
}

static int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// contiguous (B, T, H, D) views
static orion::AttnParams attn_shape(int B, int T, int Tk, int Hq, int Hkv, int D) {
  orion::AttnParams p{};
  p.B = B, p.T = T, p.Tk = Tk, p.Hq = Hq, p.Hkv = Hkv;
  p.q_sh = p.k_sh = p.v_sh = p.o_sh = p.do_sh = D;
  p.q_st = p.o_st = p.do_st = (long)Hq * D;
  p.k_st = p.v_st = (long)Hkv * D;
  p.q_sb = p.o_sb = p.do_sb = p.q_st * T;
  p.k_sb = p.v_sb = p.k_st * Tk;
  return p;
}

static void check_fwd_plan(const orion::AttnParams& p, int D, bool causal, const orion::AttnSwitches& s, int qb64,
                           bool kv_over32) {
  const AttnLaunch l = orion::attn_fwd_plan(p, D, causal, s, qb64);
  const int g128 = cdiv(p.T, 128) * p.B * p.Hq, g256 = cdiv(p.T, 256) * p.B * p.Hq, lds = 4 * 64 * D * 2;
  if (D != 64 && D != 128)
    CHECK(l.kernel == -1);
  else if (s.fwd_v2 || kv_over32)
    CHECK(is_launch(l, orion::ATTN_FWD64, g128, 256, lds));
  else if (D == 64 && causal && s.fwd_diag)
    CHECK(is_launch(l, orion::ATTN_FWD3_STAMPED, g256, 256, 32768));
  else if (D == 64 && causal && !s.fwd_v3)
    CHECK(is_launch(l, orion::ATTN_FWD4, g128, 256, 32768));
  else if (D == 64 && qb64 == 2)
    CHECK(is_launch(l, orion::ATTN_FWD3_QB2, g256, 256, 32768));
  else
    CHECK(is_launch(l, orion::ATTN_FWD3_QB1, g128, 256, lds));
}

static void check_bwd_plan(const orion::AttnParams& p, int D, bool causal, int flags, bool want_bias,
                           const orion::AttnSwitches& s, bool over32) {
  const orion::AttnBwdPlan r = orion::attn_bwd_plan(p, D, causal, flags, want_bias, s);
  if (D != 64 && D != 128) {
    CHECK(r.form == -1);
    return;
  }
  const int delta_grid = cdiv((long)p.B * p.Hq * p.T * (D / 8), 256);
  const int kv_grid = cdiv(p.Tk, 128) * p.B * p.Hkv, dq_grid = cdiv(p.T, 128) * p.B * p.Hq;
  const bool split = ((flags & 4) || !(flags & 8)) && !over32;
  if (!split) {
    CHECK(r.form == orion::ATTN_FUSED && !r.bias_in_kernel && r.n == 2);
    CHECK(is_launch(r.step[0], orion::ATTN_BWD_PRE, delta_grid, 256, 0));
    CHECK(is_launch(r.step[1], orion::ATTN_BWD, kv_grid, 256, D == 64 ? 78336 : 147968));
    return;
  }
  const bool bias = want_bias && D == 64 && p.T == p.Tk && p.Hq == p.Hkv && p.T % 32 == 0;
  CHECK(r.form == orion::ATTN_SPLIT && r.bias_in_kernel == bias);
  const int kv_lds = 2 * 2 * 32 * D * 2 + 4 * 32 * 4 + (D == 128 ? 32 * 4 * D * 2 : 0), dq_lds = 4 * 64 * D * 2;
  CHECK(kv_lds == (D == 64 ? 16896 : 66048));
  if (D == 64 && s.bwd_diag) {
    CHECK(r.n == 2 && is_launch(r.step[0], orion::ATTN_DELTA, delta_grid, 256, 0) &&
          is_launch(r.step[1], orion::ATTN_KV_STAMPED, kv_grid, 256, kv_lds));
  } else if (D == 64 && !s.dq_v3) {
    CHECK(r.n == 2 && is_launch(r.step[0], bias ? orion::ATTN_DQ4_BIAS : orion::ATTN_DQ4, dq_grid, 256, 32768) &&
          is_launch(r.step[1], orion::ATTN_KV, kv_grid, 256, kv_lds));
  } else if (D == 128 && !s.delta_pass) {
    CHECK(r.n == 2 && is_launch(r.step[0], orion::ATTN_DQ_FD, dq_grid, 256, dq_lds) &&
          is_launch(r.step[1], orion::ATTN_KV, kv_grid, 256, kv_lds));
  } else {
    CHECK(r.n == 3 && is_launch(r.step[0], bias ? orion::ATTN_DELTA_BIAS : orion::ATTN_DELTA, delta_grid, 256, 0) &&
          is_launch(r.step[1], orion::ATTN_KV, kv_grid, 256, kv_lds) &&
          is_launch(r.step[2], bias ? orion::ATTN_DQ_BIAS : orion::ATTN_DQ, dq_grid, 256, dq_lds));
  }
}

static void check_attention_plans() {
  // the switches: the documented values, read once
  setenv("ORION_ATTN_FWD", "v3", 1);
  setenv("ORION_ATTN_DQ", "v3", 1);
  setenv("ORION_ATTN_DELTA", "pass", 1);
  setenv("ORION_ATTN_DIAG", "0", 1);
  unsetenv("ORION_ATTN_FWD_DIAG");
  const orion::AttnSwitches env = orion::attn_switches();
  CHECK(!env.fwd_v2 && env.fwd_v3 && env.dq_v3 && env.delta_pass && !env.fwd_diag && !env.bwd_diag);
  setenv("ORION_ATTN_FWD", "v2", 1);
  CHECK(!orion::attn_switches().fwd_v2);  // not read again

  for (int sw = 0; sw < 64; ++sw) {
    const orion::AttnSwitches s{bool(sw & 1), bool(sw & 2), bool(sw & 4), bool(sw & 8), bool(sw & 16), bool(sw & 32)};
    for (int D : {64, 128, 96})
      for (bool causal : {false, true}) {
        for (int Hkv : {4, 2})          // MHA, GQA
          for (int T : {160, 300})      // T % 32 == 0 and not; 2 and 3 tiles of 128
            for (int Tk : {T, T + 100}) {
              const orion::AttnParams p = attn_shape(2, T, Tk, 4, Hkv, D);
              for (int qb64 : {1, 2}) check_fwd_plan(p, D, causal, s, qb64, false);
              for (int flags : {0, 4, 8})
                for (bool want_bias : {false, true}) check_bwd_plan(p, D, causal, flags, want_bias, s, false);
            }
        // operands just below and at the 2^31-byte limit of the 32-bit offsets: 65 tokens whose last row
        // starts 64 strides in, so ((T - 1) * stride + (Hq - 1) * D + D) * 2 == 2^31 at the strides below
        if (D == 96) continue;
        const long kv_at = ((1L << 30) - D) / 64, q_at = ((1L << 30) - 4 * D) / 64;
        for (int which = 0; which < 4; ++which)
          for (int below : {1, 0}) {
            orion::AttnParams p = attn_shape(2, 65, 65, 4, 2, D);
            (which == 0 ? p.k_st : which == 1 ? p.v_st : which == 2 ? p.q_st : p.do_st) =
                (which < 2 ? kv_at : q_at) - below;
            check_fwd_plan(p, D, causal, s, 2, which < 2 && !below);
            for (int flags : {0, 4, 8}) check_bwd_plan(p, D, causal, flags, true, s, !below);
          }
      }
  }
  // the (D, causal) -> template argument helper
  for (int D : {64, 128, 96})
    for (bool causal : {false, true}) {
      const int r = orion::attn_dispatch(D, causal, [](auto d, auto c) { return d() * 2 + (c() ? 1 : 0); });
      CHECK(r == (D == 96 ? -1 : D * 2 + (causal ? 1 : 0)));
    }
}

int main() {
  check_attention_plans();
  // split-K planning over the shapes the models produce (and odd ones)
  const int Ms[] = {32, 96, 256, 4096, 8192, 8224, 16384, 65536, 131072, 262144};
  const int Ns[] = {8, 64, 264, 768, 1000, 2304, 3072, 4096, 11008, 50304};
  for (int M : Ms)
    for (int n1 : Ns)
      for (int n2 : Ns) {
        const int S = orion_wgrad_splits(M, n1, n2);
        CHECK(S >= 1 && S <= 32);
        CHECK(orion_wgrad_effective_splits(M, S) == S);
        for (int req = 1; req <= 40; req += 3) {
          const int e = orion_wgrad_effective_splits(M, req);
          CHECK(e >= 1 && e <= req);
        }
      }
  // tail split: head rows are the whole tile rows inside the whole rounds, the tail (a partial
  // last tile row allowed) at most half a round
  for (int M : Ms)
    for (int n1 : Ns)
      for (int n2 : Ns) {
        int S2 = 0;
        const int R1 = orion_wgrad_tail_rows(M, n1, n2, &S2);
        CHECK(R1 >= 0 && R1 < n1 && R1 % 256 == 0);
        if (R1 > 0) {
          const long t1 = (n1 + 255) / 256, t2 = (n2 + 255) / 256, tiles = t1 * t2;
          const long head = (long)(R1 / 256) * t2, tail = tiles - head, whole = tiles / 256 * 256;
          CHECK(head <= whole && head > whole - t2 && tail > 0 && tail <= 128);
          CHECK(S2 >= 2 && tail * S2 <= 256 && orion_wgrad_effective_splits(M, S2) == S2);
        } else {
          CHECK(S2 == 1);
        }
      }
  {  // Llama-7B gate_up weight gradient at 16k tokens: 80 tile rows unsplit + 6 rows at S2 = 2
    int S2 = 0;
    CHECK(orion_wgrad_tail_rows(16384, 22016, 4096, &S2) == 80 * 256 && S2 == 2);
    CHECK(orion_wgrad_tail_rows(16384, 12288, 4096, &S2) == 0);  // 768 tiles: whole rounds
    // GPT-2's LM head at 4k tokens: 170 tile rows unsplit, 26.5 rows at S2 = 3
    CHECK(orion_wgrad_tail_rows(4096, 50304, 768, &S2) == 170 * 256 && S2 == 3);
  }
  // scratch sizing is monotone and positive
  for (int rows = 1; rows < (1 << 20); rows = rows * 3 + 1) {
    CHECK(orion_layernorm_bwd_blocks(rows) >= 1 && orion_layernorm_bwd_blocks(rows) <= 1024);
    CHECK(orion_rmsnorm_bwd_blocks(rows) >= 1);
    CHECK(orion_colsum_scratch(rows, 768) >= 768);
  }
  // the exported scratch sizes are, to the float, the expressions their callers used to write out
  // (the fold's mid scratch as literal multiples of its 16 splits)
  for (int rows : {1, 63, 64, 65, 4096, 65536, 70000})
    for (int C : {64, 768, 4096}) {
      const long nb = orion_layernorm_bwd_blocks(rows), rb = orion_rmsnorm_bwd_blocks(rows);
      const long prow = rows, ld = C;  // attn_bwd's bias partials: prow 32-token blocks of ld columns
      CHECK(orion_layernorm_bwd_scratch(rows, C) == 3 * nb * C + 48L * C);
      CHECK(orion_rmsnorm_bwd_scratch(rows, C) == (rb + 32) * C);
      CHECK(orion_colsum_scratch(rows, C) == (nb + 32) * C);
      CHECK(prow * ld + orion_colsum_mid_scratch((int)ld, 1) == prow * ld + 16 * ld);
    }
  // argument validation: every one of these must be rejected without a launch
  std::vector<uint16_t> buf(1 << 16);
  const void* p = buf.data();
  const void* mis = reinterpret_cast<const char*>(buf.data()) + 2;  // not 16-byte aligned
  void* o = buf.data();
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 48, 0, 0, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -1);   // K % 64
  CHECK(orion_gemm(p, 64, p, 64, 64, 60, 64, 0, 0, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -1);   // N % 8
  CHECK(orion_gemm(p, 66, p, 64, 64, 64, 64, 0, 0, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -1);   // ld % 8
  CHECK(orion_gemm(mis, 64, p, 64, 64, 64, 64, 0, 0, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -2); // alignment
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 0, 1, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -3);   // bias missing
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 0, 2, o, 64, p, nullptr, 64, nullptr, 0, 0) == -3);        // gelu out2 missing
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 1, 3, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -3);   // pre missing
  CHECK(orion_gemm(p, 64, p, 64, 0, 64, 64, 0, 0, o, 64, nullptr, nullptr, 0, nullptr, 0, 0) == -1);    // M = 0
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 0, 5, o, 128, nullptr, o, 128, p, 128, 0) == -3);         // swiglu: NN only
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 1, 5, o, 128, nullptr, nullptr, 0, p, 128, 0) == -3);     // swiglu: out2 missing
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 1, 5, o, 128, nullptr, o, 128, nullptr, 0, 0) == -3);     // swiglu: pre missing
  float part[4096];
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 1, 0, o, 64, nullptr, nullptr, 0, nullptr, 0, 0, o, 0, part) == -3);  // db needs epi 3
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 1, 3, o, 64, nullptr, nullptr, 0, p, 64, 0, o, 0, nullptr) == -3);  // db needs scratch
  CHECK(orion_gemm(p, 64, p, 64, 64, 64, 64, 1, 3, o, 72, nullptr, nullptr, 0, p, 64, 0, o, 0, part) == -3);     // db needs ldo == N
  CHECK(orion_gemm_colsum_scratch(65, 64) == (2 + 32) * 64);
  CHECK(orion_wgrad(p, 64, p, 64, 33, 64, 64, 1, nullptr, o, nullptr, 0, 0, 0, 0) == -1);              // M % BK
  CHECK(orion_wgrad(mis, 64, p, 64, 64, 64, 64, 1, nullptr, o, nullptr, 0, 0, 0, 0) == -2);            // alignment
  CHECK(orion_wgrad(p, 64, p, 64, 4096, 64, 64, 2, nullptr, o, nullptr, 0, 0, 0, 0) == -4);            // slabs missing
  if (failures) return 1;
  std::printf("host logic ok\n");
  return 0;
}
