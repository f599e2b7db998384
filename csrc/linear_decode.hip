// Skinny linear layer for the decode step on gfx950 (wave64, bf16 in / out, fp32 accumulation):
//   y[M, Nout] = epi(pro(x)[M, K] . W[N, K]^T),  1 <= M <= 16.
//
// At M <= 16 a linear layer is a stream of its weight: every byte of W is used by exactly one
// wave, once.  linear_decode_kernel<NORM, ACT, NW, U>, grid ceil(Nout / 16), 64 NW threads:
//   * one workgroup per 16 output columns; v_mfma_f32_16x16x32_bf16 with x as the A operand,
//     zero-padded in registers to 16 rows, and W^T as the B operand: lane l holds
//     W[n0 + (l & 15)][k + 8 (l >> 4) .. + 8], which is one 16-byte load of a row-major W row,
//     so the weights go from memory to VGPRs and straight into the MFMA (no LDS round trip);
//   * K is cut into chunks of U MFMA steps (32 U elements) that the NW waves take in turn, so
//     the workgroup reads NW x 64 U contiguous bytes of each of its rows per round; the next
//     chunk's loads are issued before the current chunk's MFMAs (two register sets, the waits
//     land on first use).  The weight loads are non-temporal (read once); x, gamma / beta, bias
//     and the residual stream use the default policy (every workgroup re-reads them from the
//     L2).  A wave's rounds are sequential memory latencies, so the plain projections (no
//     prologue, no activation: the residual sites, small N and the longest K) with K >= 2048
//     run 8 waves x 8 steps -- a round covers 2048 elements of K -- and everything else, a
//     short K or a stage that also holds x and gamma / beta, 4 waves x 4 steps (a round of
//     512; at K = 768 the wide form measured 1 us slower, its waves 3-7 idle);
//   * prologue (NORM): LayerNorm or RMSNorm of the rows of x.  Every workgroup recomputes the
//     statistics of the <= 16 rows (16 threads per row, fp32, two passes for LayerNorm) and the
//     A fragments are normalised on the fly and rounded to bf16, where the unfused norm kernel
//     rounds its output;
//   * the waves' fp32 partial tiles are summed through LDS in wave order (no atomics: the
//     result is bit-reproducible), then the epilogue runs in fp32 on one (row, column) per
//     thread (its bias and residual values loaded before the K loop): + bias, GELU-tanh or
//     SwiGLU, + residual, one rounding at the store.  With SwiGLU the workgroup streams rows n
//     and Nout + n of the packed [gate; up] weight (two B fragments per step on the same A) and
//     stores silu(g) u;
//   * nothing is read beyond row M - 1, weight row N - 1 or element K - 1 (K % 8 == 0, so an
//     8-element fragment is inside or outside as a whole); padded fragments are zeros.
#include "common.h"
#include "launchers.h"
#include "linear_decode_mfma.h"

namespace orion {

namespace {

// waves per workgroup and MFMA k-steps (16-byte loads per operand and lane) per chunk
constexpr int LD_NW_WIDE = 8, LD_U_WIDE = 8;  // plain projections with K >= LD_K_WIDE
constexpr int LD_NW = 4, LD_U = 4;            // the others
constexpr int LD_K_WIDE = 32 * LD_NW_WIDE * LD_U_WIDE;  // one full round of the wide form

template <int NORM, int NB, int U>
struct LdStage {
  bf16x8 w[NB][U];
  bf16x8 x[U];
  bf16x8 g[NORM != LD_NORM_NONE ? U : 1];
  bf16x8 b[NORM == LD_NORM_LAYER ? U : 1];
};

}  // namespace

template <int NORM, int ACT, int NW, int U>
__global__ __launch_bounds__(64 * NW) void linear_decode_kernel(const LinearDecodeParams p) {
  constexpr int NB = ACT == LD_ACT_SWIGLU ? 2 : 1, KC = 32 * U;  // KC: elements of K per chunk
  static_assert(NW >= 4 && (NORM == LD_NORM_NONE || NW == 4), "the statistics and the epilogue use 256 threads");
  typedef LdStage<NORM, NB, U> Stage;
  __shared__ float part[NW][NB][16][16];
  __shared__ float stats[16][2];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;  // A row / B column of this lane, its 8-element k group
  const int M = p.M, K = p.K, Nout = p.Nout;
  const long n0 = (long)blockIdx.x * 16;
  const bool n_ok = n0 + c < Nout, m_ok = c < M;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const bf16_t* wrow[NB];
#pragma unroll
  for (int h = 0; h < NB; ++h) wrow[h] = p.w + ((long)h * Nout + n0 + c) * K;
  const bf16_t* xrow = p.x + (long)c * p.x_rs;

  auto load_stage = [&](int k0, Stage& s) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kk = k0 + u * 32 + g * 8;
      const bool k_ok = kk < K;
      ORION_DASSERT(!k_ok || kk + 8 <= K);
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        s.w[h][u] = zero;
        if (k_ok && n_ok) {
          ORION_DASSERT((long)h * Nout + n0 + c < (long)NB * Nout);
          s.w[h][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wrow[h] + kk));
        }
      }
      s.x[u] = zero;
      if (k_ok && m_ok) s.x[u] = *reinterpret_cast<const bf16x8*>(xrow + kk);
      if constexpr (NORM != LD_NORM_NONE) {
        s.g[u] = zero;
        if (k_ok) s.g[u] = *reinterpret_cast<const bf16x8*>(p.norm_w + kk);
      }
      if constexpr (NORM == LD_NORM_LAYER) {
        s.b[u] = zero;
        if (k_ok && p.norm_b) s.b[u] = *reinterpret_cast<const bf16x8*>(p.norm_b + kk);
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
      bf16x8 a = cur.x[u];
      if constexpr (NORM != LD_NORM_NONE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float o = (bf2f(cur.x[u][j]) - mean) * rstd * bf2f(cur.g[u][j]);
          if constexpr (NORM == LD_NORM_LAYER) o += bf2f(cur.b[u][j]);
          a[j] = f2bf(o);
        }
        if (!m_ok) a = zero;  // a padded row is zeros, not beta
      }
#pragma unroll
      for (int h = 0; h < NB; ++h) acc[h] = ld_mfma(a, cur.w[h][u], acc[h]);
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
static int launch_linear_decode(const LinearDecodeParams& p, hipStream_t st) {
  const long tiles = ((long)p.Nout + 15) / 16;
  const dim3 grid((unsigned)tiles);
  if (p.act == LD_ACT_NONE) {
    if (NORM == LD_NORM_NONE && p.K >= LD_K_WIDE) {
      if constexpr (NORM == LD_NORM_NONE)
        linear_decode_kernel<NORM, LD_ACT_NONE, LD_NW_WIDE, LD_U_WIDE><<<grid, 64 * LD_NW_WIDE, 0, st>>>(p);
    } else {
      linear_decode_kernel<NORM, LD_ACT_NONE, LD_NW, LD_U><<<grid, 64 * LD_NW, 0, st>>>(p);
    }
  } else if (p.act == LD_ACT_GELU) {
    linear_decode_kernel<NORM, LD_ACT_GELU, LD_NW, LD_U><<<grid, 64 * LD_NW, 0, st>>>(p);
  } else {
    linear_decode_kernel<NORM, LD_ACT_SWIGLU, LD_NW, LD_U><<<grid, 64 * LD_NW, 0, st>>>(p);
  }
  return (int)hipGetLastError();
}

// No allocation, synchronisation or copy: the launch is captured into the decode step's graph.
int orion_linear_decode(const LinearDecodeParams& p, hipStream_t st) {
  if (p.M < 1 || p.M > 16 || p.Nout < 1 || p.K < 8 || p.K % 8) return -1;
  if (p.norm < LD_NORM_NONE || p.norm > LD_NORM_RMS || p.act < LD_ACT_NONE || p.act > LD_ACT_SWIGLU) return -2;
  if (!p.x || !p.w || !p.y || (p.norm != LD_NORM_NONE && !p.norm_w)) return -3;
  if (p.norm != LD_NORM_LAYER && p.norm_b) return -4;
  if (p.norm == LD_NORM_NONE) return launch_linear_decode<LD_NORM_NONE>(p, st);
  if (p.norm == LD_NORM_LAYER) return launch_linear_decode<LD_NORM_LAYER>(p, st);
  return launch_linear_decode<LD_NORM_RMS>(p, st);
}
