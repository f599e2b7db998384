// Generation-time attention for gfx950 (wave64, bf16 in, fp32 math): single-query attention
// over a key/value cache, split over keys, and the cache append (optionally with RoPE).
//
// attn_decode_kernel<D, NR>, grid (splits, Hkv, B), 256 threads:
//   * decode is a memory-bound stream of K and V, so one workgroup serves all G = Hq / Hkv query
//     heads of its KV head (K / V leave memory once per KV head, not once per query head), NR <= 8
//     rows at a time (the groups are looped when G > 8: the second pass hits the L2);
//   * a key row is D bf16 = D / 8 lanes of one 16-byte load each, so a wave's load instruction
//     covers 64 / (D / 8) keys; every wave walks its own keys with U loads of K and of V in
//     flight and the next tile's loads issued before the current tile's math (K / V go straight
//     to VGPRs: no LDS staging -- each byte is used by exactly one wave);
//   * q stays packed bf16 (4 VGPRs per row) and q.k is v_dot2_f32_bf16 on the packed words,
//     summed over the D / 8 lanes of the key by DPP moves;
//   * every (wave, key slot) keeps its own online softmax in base 2 (running max, sum, and the
//     8 output columns of its lane per row); they are merged once at the end: by shuffles inside
//     a wave, then through LDS across the four waves -- fixed order, no atomics, so the result is
//     bit-reproducible;
//   * the length is read on the device (kv_lens[b], clamped to [0, Tmax]); keys at or beyond it
//     are never loaded and their scores are -inf by select, so stale NaN / Inf there cannot
//     reach the result.  A (row, split) without keys yields the neutral partial (-inf, 0, 0);
//     every exp2 argument subtracts a max that -inf has been replaced in, so no inf - inf;
//   * splits == 1 writes bf16 o; otherwise fp32 partials (m, l, o[D]) per (b, head, split) that
//     attn_decode_combine_kernel merges.
//
// kv_append_kernel: one thread per 8 rotation pairs (two 16-byte loads and stores) of a head
// of q | k_new | v_new; k (rotated in fp32 at position kv_lens[b] + t when tables are given,
// rounded once) and v (copied bit for bit) land in the cache, the rotated q in a contiguous
// output.  Positions outside [0, Tmax) are skipped (their q rows are zero).
#include "common.h"
#include "attn_decode_lanes.h"
#include "launchers.h"

namespace orion {

namespace {

constexpr int DEC_U = 4;   // K (and V) loads in flight per wave and tile

template <int D>
struct DecodeShape {
  static constexpr int LPK = D / 8;                  // lanes per key row
  static constexpr int KPW = 64 / LPK;               // keys per wave-wide load
  static constexpr int TILE = DEC_NW * DEC_U * KPW;  // keys per workgroup iteration
};

}  // namespace

template <int D, int NR>
__global__ __launch_bounds__(256) void attn_decode_kernel(const DecodeParams p) {
  typedef DecodeShape<D> S;
  constexpr int LPK = S::LPK, KPW = S::KPW, TILE = S::TILE, U = DEC_U, NW = DEC_NW;
  __shared__ float sm[NW][NR][D + 2];  // per wave and row: o[D], m, l

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane % LPK, kg = lane / LPK;
  const int G = p.Hq / p.Hkv;
  ORION_DASSERT(b < p.B && hk < p.Hkv && split < p.splits);

  int len = p.kv_lens[b];
  len = len < 0 ? 0 : (len > p.Tmax ? p.Tmax : len);
  const int k0 = split * p.chunk;
  const int k1 = min(k0 + p.chunk, len);  // k1 <= k0: this split has no keys for row b
  const bf16_t* kb = p.k + (long)b * p.k_sb + (long)hk * p.k_sh + c * 8;
  const bf16_t* vb = p.v + (long)b * p.v_sb + (long)hk * p.v_sh + c * 8;

  auto load_tile = [&](int base, bf16x8(&kk)[U], bf16x8(&vv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * KPW + kg;
      kk[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      vv[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (key < k1) {
        ORION_DASSERT(key >= 0 && key < p.Tmax);
        kk[u] = *reinterpret_cast<const bf16x8*>(kb + (long)key * p.k_st);
        vv[u] = *reinterpret_cast<const bf16x8*>(vb + (long)key * p.v_st);
      }
    }
  };

  for (int g0 = 0; g0 < G; g0 += NR) {
    bf16x8 qv[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      qv[r] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (g0 + r < G) {
        const int hq = hk * G + g0 + r;
        ORION_DASSERT(hq < p.Hq);
        qv[r] = *reinterpret_cast<const bf16x8*>(p.q + (long)b * p.q_sb + (long)hq * p.q_sh + c * 8);
      }
    }
    float m[NR], l[NR], acc[NR][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      m[r] = -INFINITY;
      l[r] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
    }

    int base = k0 + w * (U * KPW);  // wave-uniform
    bf16x8 kc[U], vc[U];
    if (base < k1) load_tile(base, kc, vc);
    for (; base < k1; base += TILE) {
      bf16x8 kn[U], vn[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { kn[u] = kc[u]; vn[u] = vc[u]; }
      if (base + TILE < k1) load_tile(base + TILE, kn, vn);  // next tile before this one's math

      float pr[NR][U];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float s[U];
        float mn = m[r];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float d = key_lanes_sum<LPK>(dot8_bf16(qv[r], kc[u]));
          // select, not a zero weight: a stale key past the length must not reach the result
          s[u] = (base + u * KPW + kg < k1) ? d * p.scale_log2 : -INFINITY;
          mn = fmaxf(mn, s[u]);
        }
        const float ms = finite_or_zero(mn);
        const float alpha = __builtin_amdgcn_exp2f(m[r] - ms);
        m[r] = mn;
        float ls = l[r] * alpha;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          pr[r][u] = __builtin_amdgcn_exp2f(s[u] - ms);
          ls += pr[r][u];
        }
        l[r] = ls;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float vf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vf[j] = bf2f(vc[u][j]);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r][j] = fmaf(pr[r][u], vf[j], acc[r][j]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) { kc[u] = kn[u]; vc[u] = vn[u]; }
    }

    // merge the key slots of this wave (lanes with equal c), then the waves through LDS
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      float mt = m[r];
#pragma unroll
      for (int o = LPK; o < 64; o <<= 1) mt = fmaxf(mt, __shfl_xor(mt, o, 64));
      const float a = __builtin_amdgcn_exp2f(m[r] - finite_or_zero(mt));
      float ls = l[r] * a;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] *= a;
#pragma unroll
      for (int o = LPK; o < 64; o <<= 1) {
        ls += __shfl_xor(ls, o, 64);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] += __shfl_xor(acc[r][j], o, 64);
      }
      if (kg == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sm[w][r][c * 8 + j] = acc[r][j];
        if (c == 0) {
          sm[w][r][D] = mt;
          sm[w][r][D + 1] = ls;
        }
      }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NR * D; idx += 256) {
      const int r = idx / D, d = idx % D;
      if (g0 + r >= G) continue;
      float mt = -INFINITY;
#pragma unroll
      for (int i = 0; i < NW; ++i) mt = fmaxf(mt, sm[i][r][D]);
      const float ms = finite_or_zero(mt);
      float lt = 0.f, ot = 0.f;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const float a = __builtin_amdgcn_exp2f(sm[i][r][D] - ms);
        lt = fmaf(a, sm[i][r][D + 1], lt);
        ot = fmaf(a, sm[i][r][d], ot);
      }
      const long head = (long)b * p.Hq + hk * G + g0 + r;
      ORION_DASSERT(head < (long)p.B * p.Hq);
      if (p.splits == 1) {
        p.o[head * D + d] = f2bf(lt > 0.f ? ot / lt : 0.f);
      } else {
        const long slot = head * p.splits + split;
        p.ws_o[slot * D + d] = ot;
        if (d == 0) {
          p.ws_ml[slot * 2] = mt;
          p.ws_ml[slot * 2 + 1] = lt;
        }
      }
    }
    __syncthreads();  // sm is reused by the next group of rows
  }
}

// o[head][d] = sum_s 2^(m_s - M) o_s[d] / sum_s 2^(m_s - M) l_s over the splits' partials.
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(const float* __restrict__ ws_o,
                                                                  const float* __restrict__ ws_ml,
                                                                  bf16_t* __restrict__ o, int splits, int D,
                                                                  long heads) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= heads * D) return;
  const long head = i / D;
  const int d = (int)(i % D);
  const float* ml = ws_ml + head * splits * 2;
  float mt = -INFINITY;
  for (int s = 0; s < splits; ++s) mt = fmaxf(mt, ml[s * 2]);
  const float ms = finite_or_zero(mt);  // all splits empty: every weight is 2^(-inf - 0) = 0
  float lt = 0.f, ot = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float a = __builtin_amdgcn_exp2f(ml[s * 2] - ms);
    lt = fmaf(a, ml[s * 2 + 1], lt);
    ot = fmaf(a, ws_o[(head * splits + s) * D + d], ot);
  }
  o[i] = f2bf(lt > 0.f ? ot / lt : 0.f);
}

__global__ __launch_bounds__(256) void kv_append_kernel(const AppendParams p) {
  const int D = p.D, P8 = D / 16;  // groups of 8 rotation pairs per head
  const int HT = p.Hq + 2 * p.Hkv;  // heads per token: q | k | v (p.Hq = 0 without q)
  const long n = (long)p.B * p.T * HT * P8;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int pg = (int)(i % P8);
    const long row = i / P8;
    const int h = (int)(row % HT);
    const int t = (int)((row / HT) % p.T);
    const int b = (int)(row / ((long)HT * p.T));
    const long pos = (long)p.kv_lens[b] + t;
    const bool ok = pos >= 0 && pos < p.Tmax;
    const bf16_t* src;
    bf16_t* dst;
    bool rot = p.cosv != nullptr;
    if (h < p.Hq) {
      src = p.q + b * p.q_sb + t * p.q_st + h * p.q_sh;
      dst = p.q_out + (((long)b * p.T + t) * p.Hq + h) * D;
      if (!ok) {  // no position to rotate at: a defined value for the skipped token
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<bf16x8*>(dst + pg * 8) = z;
        *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = z;
        continue;
      }
    } else {
      if (!ok) continue;  // never written
      const int hh = h - p.Hq;
      if (hh < p.Hkv) {
        src = p.k_new + b * p.kn_sb + t * p.kn_st + hh * p.kn_sh;
        dst = p.k_cache + b * p.kc_sb + pos * p.kc_st + hh * p.kc_sh;
      } else {
        src = p.v_new + b * p.vn_sb + t * p.vn_st + (hh - p.Hkv) * p.vn_sh;
        dst = p.v_cache + b * p.vc_sb + pos * p.vc_st + (hh - p.Hkv) * p.vc_sh;
        rot = false;
      }
    }
    const bf16x8 lo = *reinterpret_cast<const bf16x8*>(src + pg * 8);
    const bf16x8 hi = *reinterpret_cast<const bf16x8*>(src + D / 2 + pg * 8);
    if (!rot) {
      *reinterpret_cast<bf16x8*>(dst + pg * 8) = lo;
      *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = hi;
      continue;
    }
    ORION_DASSERT(pos < p.npos);
    const float* cr = p.cosv + pos * (D / 2) + pg * 8;
    const float* sr = p.sinv + pos * (D / 2) + pg * 8;
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr), c1 = *reinterpret_cast<const f32x4*>(cr + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
    bf16x8 o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float cc = j < 4 ? c0[j] : c1[j - 4];
      const float ss = j < 4 ? s0[j] : s1[j - 4];
      const float x1 = bf2f(lo[j]), x2 = bf2f(hi[j]);
      o1[j] = f2bf(x1 * cc - x2 * ss);
      o2[j] = f2bf(x2 * cc + x1 * ss);
    }
    *reinterpret_cast<bf16x8*>(dst + pg * 8) = o1;
    *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = o2;
  }
}

}  // namespace orion

using namespace orion;

static int orion_attn_decode_tile(int D) { return D == 64 ? DecodeShape<64>::TILE : DecodeShape<128>::TILE; }

// Splits chosen on the host from the caller's upper bound on the length (the cache view's
// Tmax): enough workgroups for two per CU of the 256 when the length allows, each split a
// whole number of key tiles of `tile` keys.  Returns the split count and the keys per split.
int orion_attn_decode_split_plan(int tile, int B, int Hkv, int Tmax, int splits, int* chunk) {
  const int tiles = Tmax > 0 ? (Tmax + tile - 1) / tile : 1;
  if (splits <= 0) {
    const long groups = (long)B * Hkv;
    long want = (512 + groups - 1) / groups;
    if (want > 128) want = 128;
    splits = (int)(want < tiles ? want : tiles);
    const int per = (tiles + splits - 1) / splits;
    *chunk = per * tile;
    return (tiles + per - 1) / per;  // no split that starts beyond Tmax
  }
  const int per = (tiles + splits - 1) / splits;
  *chunk = per * tile;
  return splits;
}

int orion_attn_decode_plan(int B, int Hkv, int Tmax, int D, int splits, int* chunk) {
  return orion_attn_decode_split_plan(orion_attn_decode_tile(D), B, Hkv, Tmax, splits, chunk);
}

// The merge of the splits' partials into bf16 o (B * Hq heads of D columns).
int orion_attn_decode_combine(const float* ws_o, const float* ws_ml, void* o, int splits, int D, long heads,
                              hipStream_t st) {
  const long n = heads * D;
  attn_decode_combine_kernel<<<(int)((n + 255) / 256), 256, 0, st>>>(ws_o, ws_ml, (bf16_t*)o, splits, D, heads);
  return (int)hipGetLastError();
}

template <int D>
static int launch_decode(const DecodeParams& p, hipStream_t st) {
  const int G = p.Hq / p.Hkv;
  const dim3 grid(p.splits, p.Hkv, p.B);
  if (G > 4) attn_decode_kernel<D, 8><<<grid, 256, 0, st>>>(p);
  else if (G > 2) attn_decode_kernel<D, 4><<<grid, 256, 0, st>>>(p);
  else if (G == 2) attn_decode_kernel<D, 2><<<grid, 256, 0, st>>>(p);
  else attn_decode_kernel<D, 1><<<grid, 256, 0, st>>>(p);
  int rc = (int)hipGetLastError();
  if (rc || p.splits == 1) return rc;
  return orion_attn_decode_combine(p.ws_o, p.ws_ml, p.o, p.splits, D, (long)p.B * p.Hq, st);
}

int orion_attn_decode(const DecodeParams& p, int D, hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (p.B <= 0 || p.Hkv <= 0 || p.Hq % p.Hkv || p.splits < 1 || p.chunk < 1) return -2;
  if (p.Hkv > 65535 || p.B > 65535) return -3;
  if (p.splits > 1 && (!p.ws_o || !p.ws_ml)) return -4;
  if ((long)p.splits * p.chunk > (1L << 30)) return -5;
  return D == 64 ? launch_decode<64>(p, st) : launch_decode<128>(p, st);
}

int orion_kv_append(const AppendParams& p, hipStream_t st) {
  if (p.D % 16) return -1;
  if ((p.cosv == nullptr) != (p.sinv == nullptr)) return -2;
  if (p.Hq > 0 && (!p.q || !p.q_out || !p.cosv)) return -3;
  const long n = (long)p.B * p.T * (p.Hq + 2 * p.Hkv) * (p.D / 16);
  if (n <= 0) return 0;
  long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  kv_append_kernel<<<(int)g, 256, 0, st>>>(p);
  return (int)hipGetLastError();
}
