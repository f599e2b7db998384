// Which attention kernels run, in which order, with which grid, block and dynamic LDS: decided here,
// as pure host functions of the shapes, strides and switches (no HIP call, nothing launched), so
// tests/native/host_logic.cpp pins every case on the CPU.  The three attention files launch what a
// plan names; csrc/bindings.cpp sizes its scratch by it.
#pragma once

#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "attn_params.h"

namespace orion {

// A/B and diagnostic switches, read from the environment once per process.
struct AttnSwitches {
  bool fwd_v2;      // ORION_ATTN_FWD=v2: the 64-bit-addressed forward of attention.hip
  bool fwd_v3;      // ORION_ATTN_FWD=v3: attn_fwd3 at D = 64 causal (default attn_fwd4)
  bool dq_v3;       // ORION_ATTN_DQ=v3: delta pass + attn_bwd_dq at D = 64 (default attn_bwd_dq4)
  bool delta_pass;  // ORION_ATTN_DELTA=pass: the separate delta pass at D = 128 (default: fused into dQ)
  bool fwd_diag;    // ORION_ATTN_FWD_DIAG=1: stamped forward, D = 64 causal (scripts/attn_fwd_stamps.py)
  bool bwd_diag;    // ORION_ATTN_DIAG=1: stamped dK/dV only, D = 64 (scripts/attn_stamps.py)
};

inline const AttnSwitches& attn_switches() {
  static const AttnSwitches s = [] {
    auto is = [](const char* name, const char* value) {
      const char* e = std::getenv(name);
      return e && std::strcmp(e, value) == 0;
    };
    return AttnSwitches{is("ORION_ATTN_FWD", "v2"),   is("ORION_ATTN_FWD", "v3"),      is("ORION_ATTN_DQ", "v3"),
                        is("ORION_ATTN_DELTA", "pass"), is("ORION_ATTN_FWD_DIAG", "1"), is("ORION_ATTN_DIAG", "1")};
  }();
  return s;
}

enum AttnKernel {
  ATTN_FWD64,         // attention.hip: attn_fwd_kernel<D, c>
  ATTN_BWD_PRE,       //                attn_bwd_pre_kernel<D>
  ATTN_BWD,           //                attn_bwd_kernel<D, c>
  ATTN_FWD3_QB1,      // attn_fwd.hip: attn_fwd3_kernel<D, c, 1>
  ATTN_FWD3_QB2,      //               attn_fwd3_kernel<64, c, 2>
  ATTN_FWD3_STAMPED,  //               attn_fwd3_kernel<64, true, 2, true>
  ATTN_FWD4,          //               attn_fwd4_kernel<true>
  ATTN_DELTA,         // attn_bwd_split.hip: attn_delta_kernel<D>
  ATTN_DELTA_BIAS,    //                     attn_delta_kernel<64, true>
  ATTN_KV,            //                     attn_bwd_kv_kernel<D, c>
  ATTN_KV_STAMPED,    //                     attn_bwd_kv_kernel<64, c, true>
  ATTN_DQ,            //                     attn_bwd_dq_kernel<D, c>
  ATTN_DQ_BIAS,       //                     attn_bwd_dq_kernel<64, c, true>
  ATTN_DQ_FD,         //                     attn_bwd_dq_kernel<128, c, false, true> (fused delta)
  ATTN_DQ4,           //                     attn_bwd_dq4_kernel<c, false>
  ATTN_DQ4_BIAS,      //                     attn_bwd_dq4_kernel<c, true>
};

struct AttnLaunch {
  int kernel;  // AttnKernel, or a negative error code (-1: head dim)
  int grid, block, lds;
};

enum AttnBwdForm { ATTN_SPLIT, ATTN_FUSED };  // attn_bwd_split.hip | attention.hip (fp32-atomic dQ)

struct AttnBwdPlan {
  int form;             // AttnBwdForm, or -1: head dim
  bool bias_in_kernel;  // the kernels fill AttnParams::bias_part (else: column sums of the packed bf16 dQKV)
  int n;
  AttnLaunch step[3];  // in stream order
};

// waves (x 32 keys) per workgroup of the fused backward.  8 waves (256 keys) halve the dQ atomics
// but measured 7 % slower at D = 64 on MI355X (8-wave barriers, more idle waves on the
// causal diagonal), and do not fit LDS at D = 128: 4 everywhere.
template <int D>
constexpr int bwd_waves() { return 4; }
// ... and of the split backward's dK/dV kernel
template <int D>
constexpr int kv_waves() { return 4; }

// dynamic LDS bytes.  Forward and dQ: [2 buffers][K | V][64 keys][D] bf16
constexpr int attn_tile_lds(int D) { return 2 * 2 * 64 * D * 2; }
constexpr int attn_fwd4_lds() { return attn_tile_lds(64); }  // attn_fwd4 / attn_bwd_dq4: D = 64
constexpr int attn_kv_lds(int D) { return 2 * 2 * 32 * D * 2 + 4 * 32 * 4 + (D == 128 ? 32 * 4 * D * 2 : 0); }
constexpr int attn_bwd_lds(int D) {
  const int nw = D == 64 ? bwd_waves<64>() : bwd_waves<128>();
  return 32 * nw * D * 2 + 4 * 32 * D * 2 + nw * 32 * 32 * 2 + 128 * 4 + nw * D * (32 + 4) * 4;
}

// a view whose last addressed row starts `last` elements in reaches past 32-bit byte offsets
inline bool attn_over32(long last, int D) { return (last + D) * 2 >= (1L << 31); }

inline int attn_tiles(int n, int tile) { return (n + tile - 1) / tile; }

// f(integral_constant<int, D>, bool_constant<causal>) for the head dims the kernels exist for
template <class F>
int attn_dispatch(int D, bool causal, F&& f) {
  auto with_d = [&](auto d) { return causal ? f(d, std::true_type{}) : f(d, std::false_type{}); };
  if (D == 64) return with_d(std::integral_constant<int, 64>{});
  if (D == 128) return with_d(std::integral_constant<int, 128>{});
  return -1;
}

// qb64: query blocks of 32 rows per wave at D = 64 (attn_fwd.hip's ATTN_FWD_QB64)
inline AttnLaunch attn_fwd_plan(const AttnParams& p, int D, bool causal, const AttnSwitches& s, int qb64) {
  if (D != 64 && D != 128) return {-1, 0, 0, 0};
  const int g128 = attn_tiles(p.T, 128) * p.B * p.Hq, g256 = attn_tiles(p.T, 256) * p.B * p.Hq;
  const int lds = attn_tile_lds(D);
  // attn_fwd.hip addresses K / V by 32-bit buffer offsets
  if (s.fwd_v2 || attn_over32((long)(p.Tk - 1) * p.k_st, D) || attn_over32((long)(p.Tk - 1) * p.v_st, D))
    return {ATTN_FWD64, g128, 256, lds};
  if (D == 64 && causal) {  // the non-causal attn_fwd4 runs out of registers at 4 waves: fwd3
    if (s.fwd_diag) return {ATTN_FWD3_STAMPED, g256, 256, lds};
    if (!s.fwd_v3) return {ATTN_FWD4, g128, 256, attn_fwd4_lds()};
  }
  if (D == 64 && qb64 == 2) return {ATTN_FWD3_QB2, g256, 256, lds};
  return {ATTN_FWD3_QB1, g128, 256, lds};
}

// flags: AttnParams::flags (4 forces split, 8 fused; split otherwise).  want_bias: the caller wants the
// QKV bias gradient.  Split order: D = 64 -- dQ (attn_bwd_dq4: writes delta and, with the bias, its K / V
// columns), then dK/dV (reads delta); D = 128 -- dQ with the fused delta, then dK/dV; with
// ORION_ATTN_DQ=v3 / ORION_ATTN_DELTA=pass -- the delta pass, dK/dV, dQ.
inline AttnBwdPlan attn_bwd_plan(const AttnParams& p, int D, bool /*causal: no launch parameter depends on it*/,
                                 int flags, bool want_bias, const AttnSwitches& s) {
  AttnBwdPlan r{};
  if (D != 64 && D != 128) {
    r.form = -1;
    return r;
  }
  auto steps = [&r](AttnLaunch a, AttnLaunch b, AttnLaunch c = {-1, 0, 0, 0}) {
    r.step[0] = a, r.step[1] = b, r.step[2] = c;
    r.n = c.kernel < 0 ? 2 : 3;
  };
  auto as = [](AttnLaunch l, int kernel) {
    l.kernel = kernel;
    return l;
  };
  const AttnLaunch delta{ATTN_DELTA, (int)(((long)p.B * p.Hq * p.T * (D / 8) + 255) / 256), 256, 0};
  // 32-bit buffer offsets: the split dQ kernel addresses one (batch, KV head)'s K / V, the dK/dV kernel
  // one batch's Q / dO over all query heads; beyond 2 GB the fused form (64-bit addressing) runs
  const bool over32 = attn_over32((long)(p.Tk - 1) * p.k_st, D) || attn_over32((long)(p.Tk - 1) * p.v_st, D) ||
                      attn_over32((long)(p.T - 1) * p.q_st + (long)(p.Hq - 1) * p.q_sh, D) ||
                      attn_over32((long)(p.T - 1) * p.do_st + (long)(p.Hq - 1) * p.do_sh, D);
  if (((flags & 8) && !(flags & 4)) || over32) {
    const int nw = D == 64 ? bwd_waves<64>() : bwd_waves<128>();
    r.form = ATTN_FUSED;
    steps(as(delta, ATTN_BWD_PRE), {ATTN_BWD, attn_tiles(p.Tk, 32 * nw) * p.B * p.Hkv, 64 * nw, attn_bwd_lds(D)});
    return r;
  }
  r.form = ATTN_SPLIT;
  // packed self-attention with the QKV bias gradient (GPT-2: D = 64, MHA)
  const bool b = r.bias_in_kernel = want_bias && D == 64 && p.T == p.Tk && p.Hq == p.Hkv && p.T % 32 == 0;
  const int nkv = D == 64 ? kv_waves<64>() : kv_waves<128>();
  const AttnLaunch kv{ATTN_KV, attn_tiles(p.Tk, 32 * nkv) * p.B * p.Hkv, nkv * 64, attn_kv_lds(D)};
  const AttnLaunch dq{ATTN_DQ, attn_tiles(p.T, 128) * p.B * p.Hq, 256, attn_tile_lds(D)};
  if (D == 64 && s.bwd_diag)  // stamps over p.dq, no dQ kernel, no bias columns
    steps(delta, as(kv, ATTN_KV_STAMPED));
  else if (D == 64 && !s.dq_v3)
    steps({b ? ATTN_DQ4_BIAS : ATTN_DQ4, dq.grid, 256, attn_fwd4_lds()}, kv);
  else if (D == 128 && !s.delta_pass)
    steps(as(dq, ATTN_DQ_FD), kv);
  else
    steps(as(delta, b ? ATTN_DELTA_BIAS : ATTN_DELTA), kv, as(dq, b ? ATTN_DQ_BIAS : ATTN_DQ));
  return r;
}

}  // namespace orion
