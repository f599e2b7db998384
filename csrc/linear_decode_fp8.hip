// Skinny linear layer for the decode step on gfx950 with an FP8 weight (wave64, bf16 x and y,
// OCP e4m3fn weight bytes with one fp32 scale per weight row, fp32 accumulation):
//   y[M, Nout] = epi(scale . (pro(x)[M, K] . Q[N, K]^T)),  1 <= M <= 16,  W[n, k] = scale[n] Q[n, k].
//
// The structure is csrc/linear_decode.hip's (read its header first); what differs:
//   * the weight stream is half the bytes.  A lane's 16-byte non-temporal load is 16 consecutive
//     k of one weight row, two MFMA k-steps.  The MFMA sums over its 32 k slots whatever k sits
//     in which, as long as A and B agree, so a block of 64 elements of K is cut 16 per lane
//     group: lane l = (g, c) holds Q[n0 + c][kb + 16 g .. + 16] (one load) and
//     x[c][kb + 16 g .. + 16] (two 16-byte loads, as are gamma and beta); the block's two
//     v_mfma_f32_16x16x32_bf16 take the low and the high 8 of both;
//   * the FP8 words become bf16 in registers (v_cvt_scalef32_pk_bf16_fp8 at scale 1: two bytes
//     of a word per instruction, exact, every e4m3 value is a bf16 value).  x is not quantised;
//   * the scale is per output row, so it factors out of the K sum and is applied once, in the
//     fp32 epilogue: v = scale[n] sum + bias (SwiGLU: scale[n] on the gate and scale[Nout + n] on
//     the up half, before the activation).  Given (Q, scale) the kernel computes what the bf16
//     kernel computes on the exact dequantised weight;
//   * U counts 64-element blocks: a chunk is 64 U elements of K.  The plain projections with
//     K >= 2048 run 8 waves x 4 blocks (chunks of 256, rounds of 2048) and the other forms
//     without a prologue 4 waves x 2 blocks (chunks of 128, rounds of 512): the K geometry of
//     the bf16 kernel's two forms with half its weight registers.  A form with a prologue runs
//     4 waves x 1 block (chunks of 64, rounds of 256): its stage also holds x and gamma / beta
//     for 64 k per block, and what these kernels gain from is waves per SIMD, not bytes in
//     flight per wave.  Measured at the Llama-2-7B and GPT-2 shapes: one block against two,
//     lm_head 28 against 37 us, qkv_proj 26 against 28, gate_up_proj 32 against 35, GPT-2's
//     c_attn / c_fc 7.4 against 7.2; three (LayerNorm) or four (RMSNorm) blocks, at two waves
//     per SIMD, lost 30 - 35 % on the same rows;
//   * K % 16 == 0, so a 16-element fragment is inside or outside as a whole.  Nothing is read
//     beyond row M - 1, weight row N - 1, scale[N - 1] or element K - 1.
#include "common.h"
#include "fp8_cvt.h"
#include "launchers.h"
#include "linear_decode_mfma.h"

namespace orion {

namespace {

// waves per workgroup and 64-element blocks (16-byte weight loads per lane) per chunk
constexpr int LQ_NW_WIDE = 8, LQ_U_WIDE = 4;  // plain projections with K >= LQ_K_WIDE
constexpr int LQ_NW = 4;                      // the others: two blocks, one with a prologue
constexpr int lq_u(int norm) { return norm == LD_NORM_NONE ? 2 : 1; }
constexpr int LQ_K_WIDE = 64 * LQ_NW_WIDE * LQ_U_WIDE;  // one full round of the wide form

template <int NORM, int NB, int U>
struct LqStage {
  u32x4 w[NB][U];   // 16 e4m3 each
  bf16x8 x[U][2];   // the same 16 k, low and high 8
  bf16x8 g[NORM != LD_NORM_NONE ? U : 1][2];
  bf16x8 b[NORM == LD_NORM_LAYER ? U : 1][2];
};

}  // namespace

template <int NORM, int ACT, int NW, int U>
__global__ __launch_bounds__(64 * NW) void linear_decode_fp8_kernel(const LinearDecodeFp8Params p) {
  constexpr int NB = ACT == LD_ACT_SWIGLU ? 2 : 1, KC = 64 * U;  // KC: elements of K per chunk
  static_assert(NW >= 4 && (NORM == LD_NORM_NONE || NW == 4), "the statistics and the epilogue use 256 threads");
  typedef LqStage<NORM, NB, U> Stage;
  __shared__ float part[NW][NB][16][16];
  __shared__ float stats[16][2];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;  // A row / B column of this lane, its 16-element k group
  const int M = p.M, K = p.K, Nout = p.Nout;
  const long n0 = (long)blockIdx.x * 16;
  const bool n_ok = n0 + c < Nout, m_ok = c < M;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const u32x4 zero_w = {0u, 0u, 0u, 0u};  // e4m3 0x00 is +0
  const unsigned char* wrow[NB];
#pragma unroll
  for (int h = 0; h < NB; ++h) wrow[h] = p.wq + ((long)h * Nout + n0 + c) * K;
  const bf16_t* xrow = p.x + (long)c * p.x_rs;

  auto load_stage = [&](int k0, Stage& s) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = k0 + u * 64 + g * 16;
      const bool k_ok = kk < K;
      ORION_DASSERT(!k_ok || kk + 16 <= K);
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        s.w[h][u] = zero_w;
        if (k_ok && n_ok) {
          ORION_DASSERT((long)h * Nout + n0 + c < (long)NB * Nout);
          s.w[h][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[h] + kk));
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
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
  float sc0 = 1.f, sc1 = 1.f, bias0 = 0.f, bias1 = 0.f, resv = 0.f;
  if (out_ok) {
    ORION_DASSERT(n < Nout);
    sc0 = p.w_scale[n];
    if (ACT == LD_ACT_SWIGLU) sc1 = p.w_scale[Nout + n];
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
#pragma unroll
      for (int i = 0; i < 2; ++i) {
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
        for (int h = 0; h < NB; ++h)
          acc[h] = ld_mfma(a, fp8x8_to_bf16(cur.w[h][u][2 * i], cur.w[h][u][2 * i + 1]), acc[h]);
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
  v = v * sc0 + bias0;
  if constexpr (ACT == LD_ACT_GELU) v = gelu_tanh_f(v);
  if constexpr (ACT == LD_ACT_SWIGLU) {
    float up = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) up += part[i][NB - 1][row][col];
    v = silu_f(v) * (up * sc1 + bias1);
  }
  v += resv;
  ORION_DASSERT(row < M && n < Nout);
  p.y[(long)row * p.y_rs + n] = f2bf(v);
}

}  // namespace orion

using namespace orion;

template <int NORM>
static int launch_linear_decode_fp8(const LinearDecodeFp8Params& p, hipStream_t st) {
  const long tiles = ((long)p.Nout + 15) / 16;
  const dim3 grid((unsigned)tiles);
  if (p.act == LD_ACT_NONE) {
    if (NORM == LD_NORM_NONE && p.K >= LQ_K_WIDE) {
      if constexpr (NORM == LD_NORM_NONE)
        linear_decode_fp8_kernel<NORM, LD_ACT_NONE, LQ_NW_WIDE, LQ_U_WIDE><<<grid, 64 * LQ_NW_WIDE, 0, st>>>(p);
    } else {
      linear_decode_fp8_kernel<NORM, LD_ACT_NONE, LQ_NW, lq_u(NORM)><<<grid, 64 * LQ_NW, 0, st>>>(p);
    }
  } else if (p.act == LD_ACT_GELU) {
    linear_decode_fp8_kernel<NORM, LD_ACT_GELU, LQ_NW, lq_u(NORM)><<<grid, 64 * LQ_NW, 0, st>>>(p);
  } else {
    linear_decode_fp8_kernel<NORM, LD_ACT_SWIGLU, LQ_NW, lq_u(NORM)><<<grid, 64 * LQ_NW, 0, st>>>(p);
  }
  return (int)hipGetLastError();
}

// No allocation, synchronisation or copy: the launch is captured into the decode step's graph.
int orion_linear_decode_fp8(const LinearDecodeFp8Params& p, hipStream_t st) {
  if (p.M < 1 || p.M > 16 || p.Nout < 1 || p.K < 16 || p.K % 16) return -1;
  if (p.norm < LD_NORM_NONE || p.norm > LD_NORM_RMS || p.act < LD_ACT_NONE || p.act > LD_ACT_SWIGLU) return -2;
  if (!p.x || !p.wq || !p.w_scale || !p.y || (p.norm != LD_NORM_NONE && !p.norm_w)) return -3;
  if (p.norm != LD_NORM_LAYER && p.norm_b) return -4;
  if (p.norm == LD_NORM_NONE) return launch_linear_decode_fp8<LD_NORM_NONE>(p, st);
  if (p.norm == LD_NORM_LAYER) return launch_linear_decode_fp8<LD_NORM_LAYER>(p, st);
  return launch_linear_decode_fp8<LD_NORM_RMS>(p, st);
}
