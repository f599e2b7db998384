// Skinny linear layer for the decode step on gfx950 with an MXFP4 weight (wave64, bf16 x and y,
// OCP e2m1 codes with one e8m0 power-of-two scale per 32 elements of K, fp32 accumulation):
//   y[M, Nout] = epi(pro(x)[M, K] . W[N, K]^T),  1 <= M <= 16,
//   W[n, k] = 2^(scale[n][k / 32] - 127) e2m1(code[n][k]).
//
// The structure is csrc/linear_decode_fp8.hip's (read its header and csrc/linear_decode.hip's
// first); what differs:
//   * the weight stream is a quarter of the bf16 bytes.  A lane's 16-byte non-temporal load is 32
//     consecutive k of one weight row: exactly one MX block, so one scale byte goes with a load.
//     A block of 128 elements of K is cut 32 per lane group: lane l = (g, c) holds
//     code[n0 + c][kb + 32 g .. + 32] and x[c][kb + 32 g .. + 32] (four 16-byte loads, as are
//     gamma and beta); the block's four v_mfma_f32_16x16x32_bf16 take the four 8-element quarters
//     (the four words of the load) of both;
//   * the codes become bf16 in registers with v_cvt_scalef32_pk_bf16_fp4, one byte (two codes) of
//     a word per instruction.  The block scale is the instruction's scale operand, the fp32 whose
//     bits are byte << 23; code x scale is a bf16 value for every scale byte in [2, 252], so the
//     conversion is exact and there is no scale in the epilogue.  Given the bytes the kernel
//     computes what the bf16 kernel computes on the exactly dequantised weight.  x is not
//     quantised;
//   * the scale bytes are one byte load per 16-byte weight load, from scale[n0 + c][kb / 32 + g].
//     The four lane groups of a block read four consecutive bytes of a scale row, so one dword
//     per lane and a byte pick by g would replace them where K % 128 == 0; that is the same number
//     of load instructions per lane and leaves K % 128 != 0 a second path, so it is not done;
//   * U counts 128-element blocks: a chunk is 128 U elements of K.  The plain projections with
//     K >= 2048 run 8 waves x 2 blocks (chunks of 256, rounds of 2048) and every other form
//     4 waves x 1 block (chunks of 128, rounds of 512).  A prologue form's stage holds x, gamma
//     and beta for 128 k per block, twice the FP8 kernel's per weight byte, and the normalisation
//     is twice the VALU work per weight byte: these forms are level with the FP8 kernel, not
//     faster, and like the FP8 ones they live on waves per SIMD.  Measured at M = 1, the builds one
//     after the other on one box (docs/PERFORMANCE.md, "MXFP4 weight-only decode"): RMSNorm forms
//     at 4 x 2, qkv_proj 25 against 34 us, gate_up_proj 32 against 41; prologue forms at 8 x 1,
//     lm_head 34 against 59, gate_up_proj 32 against 44; the wide form at 8 x 4, o_proj 6.9
//     against 7.5, down_proj 11.3 against 12.2, and at 8 x 1, down_proj 11.3 against 13.6 (but
//     20 against 18 at M = 16).  lm_head (K = 768: six chunks on four waves) stays 10 - 16 %
//     behind the FP8 kernel, whose chunks of 64 split it evenly;
//   * K % 32 == 0, so a 32-element fragment is inside or outside as a whole.  Nothing is read
//     beyond row M - 1, code row N - 1, scale[N - 1][K / 32 - 1] or element K - 1.
#include "common.h"
#include "fp4_cvt.h"
#include "launchers.h"
#include "linear_decode_mfma.h"

namespace orion {

namespace {

// waves per workgroup and 128-element blocks (16-byte weight loads per lane) per chunk
constexpr int LX_NW_WIDE = 8, LX_U_WIDE = 2;  // plain projections with K >= LX_K_WIDE
constexpr int LX_NW = 4, LX_U = 1;            // the others
constexpr int LX_K_WIDE = 128 * LX_NW_WIDE * LX_U_WIDE;  // one full round of the wide form

template <int NORM, int NB, int U>
struct LxStage {
  u32x4 w[NB][U];      // 32 e2m1 codes each
  unsigned sc[NB][U];  // their e8m0 scale byte
  bf16x8 x[U][4];      // the same 32 k, in quarters of 8
  bf16x8 g[NORM != LD_NORM_NONE ? U : 1][4];
  bf16x8 b[NORM == LD_NORM_LAYER ? U : 1][4];
};

}  // namespace

template <int NORM, int ACT, int NW, int U>
__global__ __launch_bounds__(64 * NW) void linear_decode_mxfp4_kernel(const LinearDecodeMxfp4Params p) {
  constexpr int NB = ACT == LD_ACT_SWIGLU ? 2 : 1, KC = 128 * U;  // KC: elements of K per chunk
  static_assert(NW >= 4 && (NORM == LD_NORM_NONE || NW == 4), "the statistics and the epilogue use 256 threads");
  typedef LxStage<NORM, NB, U> Stage;
  __shared__ float part[NW][NB][16][16];
  __shared__ float stats[16][2];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;  // A row / B column of this lane, its 32-element k group
  const int M = p.M, K = p.K, Nout = p.Nout;
  const long n0 = (long)blockIdx.x * 16;
  const bool n_ok = n0 + c < Nout, m_ok = c < M;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const u32x4 zero_w = {0u, 0u, 0u, 0u};  // e2m1 code 0 is +0
  const unsigned char* wrow[NB];
  const unsigned char* srow[NB];
#pragma unroll
  for (int h = 0; h < NB; ++h) {
    wrow[h] = p.wq + ((long)h * Nout + n0 + c) * (K / 2);
    srow[h] = p.w_scale + ((long)h * Nout + n0 + c) * (K / 32);
  }
  const bf16_t* xrow = p.x + (long)c * p.x_rs;

  auto load_stage = [&](int k0, Stage& s) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = k0 + u * 128 + g * 32;
      const bool k_ok = kk < K;
      ORION_DASSERT(!k_ok || kk + 32 <= K);
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        s.w[h][u] = zero_w;
        s.sc[h][u] = 127u;  // 2^0
        if (k_ok && n_ok) {
          ORION_DASSERT((long)h * Nout + n0 + c < (long)NB * Nout && kk / 32 < K / 32);
          s.w[h][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[h] + kk / 2));
          s.sc[h][u] = srow[h][kk / 32];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s.x[u][i] = zero;
        if (k_ok && m_ok) s.x[u][i] = *reinterpret_cast<const bf16x8*>(xrow + kk + 8 * i);
        if constexpr (NORM != LD_NORM_NONE) {
          s.g[u][i] = zero;
          if (k_ok) s.g[u][i] = *reinterpret_cast<const bf16x8*>(p.norm_w + kk + 8 * i);
        }
        if constexpr (NORM == LD_NORM_LAYER) {
          s.b[u][i] = zero;
          if (k_ok && p.norm_b) s.b[u][i] = *reinterpret_cast<const bf16x8*>(p.norm_b + kk + 8 * i);
        }
      }
    }
  };

  // the first chunk's loads fly while the statistics are computed
  int k0 = wv * KC;  // wave-uniform
  Stage cur;
  if (k0 < K) load_stage(k0, cur);

  // this thread's epilogue operands, (row, col) = (thread / 16, thread % 16) of the first 256
  const int row = (threadIdx.x >> 4) & 15, col = threadIdx.x & 15;
  const long n = n0 + col;
  const bool out_ok = threadIdx.x < 256 && row < M && n < Nout;
  float bias0 = 0.f, bias1 = 0.f, resv = 0.f;
  if (out_ok) {
    ORION_DASSERT(n < Nout);
    if (p.bias) bias0 = bf2f(p.bias[n]);
    if (ACT == LD_ACT_SWIGLU && p.bias) bias1 = bf2f(p.bias[Nout + n]);
    if (p.res) resv = bf2f(p.res[(long)row * p.res_rs + n]);
  }

  float mean = 0.f, rstd = 1.f;
  if constexpr (NORM != LD_NORM_NONE) {
    const int sub = threadIdx.x & 15;  // 16 threads per row
    const bf16_t* xr = p.x + (long)row * p.x_rs;
    const float invK = 1.f / (float)K;
    float s = 0.f;
    if (row < M) {
      for (int k = sub * 8; k < K; k += 128) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = bf2f(v[j]);
          s += NORM == LD_NORM_LAYER ? f : f * f;
        }
      }
    }
    s = sum16(s);
    float mu = 0.f, q = s;
    if constexpr (NORM == LD_NORM_LAYER) {
      mu = s * invK;
      q = 0.f;
      if (row < M) {
        for (int k = sub * 8; k < K; k += 128) {
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + k);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float d = bf2f(v[j]) - mu;
            q += d * d;
          }
        }
      }
      q = sum16(q);
    }
    if (sub == 0) {
      stats[row][0] = mu;
      stats[row][1] = rsqrtf(q * invK + p.eps);
    }
    __syncthreads();
    mean = stats[c][0];
    rstd = stats[c][1];
  }

  f32x4 acc[NB];
#pragma unroll
  for (int h = 0; h < NB; ++h) acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (; k0 < K; k0 += NW * KC) {
    Stage nxt = cur;
    if (k0 + NW * KC < K) load_stage(k0 + NW * KC, nxt);  // next chunk before this one's math
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float sc[NB];
#pragma unroll
      for (int h = 0; h < NB; ++h) sc[h] = e8m0_to_f32(cur.sc[h][u]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bf16x8 a = cur.x[u][i];
        if constexpr (NORM != LD_NORM_NONE) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float o = (bf2f(cur.x[u][i][j]) - mean) * rstd * bf2f(cur.g[u][i][j]);
            if constexpr (NORM == LD_NORM_LAYER) o += bf2f(cur.b[u][i][j]);
            a[j] = f2bf(o);
          }
          if (!m_ok) a = zero;  // a padded row is zeros, not beta
        }
#pragma unroll
        for (int h = 0; h < NB; ++h) acc[h] = ld_mfma(a, fp4x8_to_bf16(cur.w[h][u][i], sc[h]), acc[h]);
      }
    }
    cur = nxt;
  }

  // C / D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int h = 0; h < NB; ++h) {
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wv][h][g * 4 + i][c] = acc[h][i];
  }
  __syncthreads();
  if (!out_ok) return;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) v += part[i][0][row][col];  // fixed order
  v += bias0;
  if constexpr (ACT == LD_ACT_GELU) v = gelu_tanh_f(v);
  if constexpr (ACT == LD_ACT_SWIGLU) {
    float up = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) up += part[i][NB - 1][row][col];
    v = silu_f(v) * (up + bias1);
  }
  v += resv;
  ORION_DASSERT(row < M && n < Nout);
  p.y[(long)row * p.y_rs + n] = f2bf(v);
}

}  // namespace orion

using namespace orion;

template <int NORM>
static int launch_linear_decode_mxfp4(const LinearDecodeMxfp4Params& p, hipStream_t st) {
  const long tiles = ((long)p.Nout + 15) / 16;
  const dim3 grid((unsigned)tiles);
  if (p.act == LD_ACT_NONE) {
    if (NORM == LD_NORM_NONE && p.K >= LX_K_WIDE) {
      if constexpr (NORM == LD_NORM_NONE)
        linear_decode_mxfp4_kernel<NORM, LD_ACT_NONE, LX_NW_WIDE, LX_U_WIDE><<<grid, 64 * LX_NW_WIDE, 0, st>>>(p);
    } else {
      linear_decode_mxfp4_kernel<NORM, LD_ACT_NONE, LX_NW, LX_U><<<grid, 64 * LX_NW, 0, st>>>(p);
    }
  } else if (p.act == LD_ACT_GELU) {
    linear_decode_mxfp4_kernel<NORM, LD_ACT_GELU, LX_NW, LX_U><<<grid, 64 * LX_NW, 0, st>>>(p);
  } else {
    linear_decode_mxfp4_kernel<NORM, LD_ACT_SWIGLU, LX_NW, LX_U><<<grid, 64 * LX_NW, 0, st>>>(p);
  }
  return (int)hipGetLastError();
}

// No allocation, synchronisation or copy: the launch is captured into the decode step's graph.
int orion_linear_decode_mxfp4(const LinearDecodeMxfp4Params& p, hipStream_t st) {
  if (p.M < 1 || p.M > 16 || p.Nout < 1 || p.K < 32 || p.K % 32) return -1;
  if (p.norm < LD_NORM_NONE || p.norm > LD_NORM_RMS || p.act < LD_ACT_NONE || p.act > LD_ACT_SWIGLU) return -2;
  if (!p.x || !p.wq || !p.w_scale || !p.y || (p.norm != LD_NORM_NONE && !p.norm_w)) return -3;
  if (p.norm != LD_NORM_LAYER && p.norm_b) return -4;
  if (p.norm == LD_NORM_NONE) return launch_linear_decode_mxfp4<LD_NORM_NONE>(p, st);
  if (p.norm == LD_NORM_LAYER) return launch_linear_decode_mxfp4<LD_NORM_LAYER>(p, st);
  return launch_linear_decode_mxfp4<LD_NORM_RMS>(p, st);
}
