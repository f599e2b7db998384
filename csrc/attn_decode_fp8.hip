// Generation-time attention over an FP8 key/value cache for gfx950 (wave64, bf16 q and o, OCP
// e4m3fn cache bytes with one fp32 scale per (row, KV head, token), fp32 math), and the
// quantising cache append.  value = scale * byte; the quantisation rule is
// orion_amd/ops/fp8.py's quantize_kv_fp8.
//
// attn_decode_fp8_kernel<D, NR>, grid (splits, Hkv, B), 256 threads: csrc/attn_decode.hip's
// attn_decode_kernel on bytes (read its header first).  The same lane geometry -- a key row is
// D / 8 lanes of 8 elements, a wave's load instruction covers 64 / (D / 8) keys, one workgroup per
// KV head serves all its query heads NR <= 8 rows at a time -- the same per-(wave, key slot)
// online softmax in base 2, the same fixed-order merge and the same combine kernel.  What differs:
//   * a lane's load is 8 bytes, half the bf16 kernel's; a wave keeps the same U = 4 loads of K
//     and of V in flight per tile, so the tile, the register budget (142 / 160 / 214 VGPRs at
//     1 / 2 / 4 query rows, 256 + 50 AGPRs at 8) and the waves per SIMD (3 / 3 / 2 / 1) are the
//     bf16 kernel's.  U = 8 (-DORION_DQ_U=8: the same bytes in flight per wave as the bf16
//     kernel, the softmax still updated per 4 key slots, per 2 at 8 rows where 4 spilled) costs
//     240 - 256 VGPRs and one or two waves per SIMD and measured slower at every shape but the
//     latency-bound one (docs/PERFORMANCE.md "FP8 KV cache"): what this kernel gains from is
//     waves per SIMD, not bytes in flight per wave;
//   * K bytes become packed bf16 (v_cvt_scalef32_pk_bf16_fp8 at scale 1, exact) for the same
//     v_dot2_f32_bf16 against the packed q, V bytes fp32 (v_cvt_pk_f32_fp8, exact);
//   * the scales are plain fp32 multiplies: score = (q . k_bytes) k_scale[key] scale_log2, and
//     the value scale folds into the weight: acc += (p v_scale[key]) v_bytes, l += p.  The
//     scales of a key are one load per lane (the D / 8 lanes of a key read one address; a wave's
//     keys are consecutive floats);
//   * bytes and scales are loaded only for keys below the length, and the scores beyond are -inf
//     by select: a stale 0x7F byte or NaN scale there cannot reach the result.
//
// kv_append_fp8_kernel<D>: kv_append_kernel's thread mapping (one thread per 8 rotation pairs:
// the lower and the upper 8 elements of a head row of q | k_new | v_new).  q is rotated and stored
// as bf16 exactly as there.  k (rotated in fp32, not rounded to bf16) and v: amax over the
// thread's 16 values and, by DPP moves, over the D / 16 adjacent lanes of the head row; scale =
// amax / 448 (1 for a zero row; an IEEE division); byte = e4m3(clamp(x / scale, -448, 448)), the
// clamp before v_cvt_pk_fp8_f32; two 8-byte stores, and lane 0 of the row stores the scale.  The
// D / 16 lanes of a row are adjacent, all inside the loop and all on the same branch together:
// the element count and the grid stride are multiples of D / 16 and the branches depend on the
// row only.
#include "common.h"
#include "attn_decode_lanes.h"
#include "fp8_cvt.h"
#include "launchers.h"

namespace orion {

namespace {

// K (and V) 8-byte loads in flight per wave and tile; -DORION_DQ_U=8 builds the measured-and-not-
// kept variant of the header
#ifndef ORION_DQ_U
#define ORION_DQ_U 4
#endif
constexpr int DQ_U = ORION_DQ_U;
static_assert(DQ_U == 4 || DQ_U == 8, "a tile is one or two softmax sub-blocks of 4 key slots");

template <int D>
struct DecodeFp8Shape {
  static constexpr int LPK = D / 8;                 // lanes per key row
  static constexpr int KPW = 64 / LPK;              // keys per wave-wide load
  static constexpr int TILE = DEC_NW * DQ_U * KPW;  // keys per workgroup iteration
};

struct Fp8Tile {
  u32x2 k[DQ_U], v[DQ_U];
  float ks[DQ_U], vs[DQ_U];
};

}  // namespace

template <int D, int NR>
__global__ __launch_bounds__(256) void attn_decode_fp8_kernel(const DecodeFp8Params p) {
  typedef DecodeFp8Shape<D> S;
  constexpr int LPK = S::LPK, KPW = S::KPW, TILE = S::TILE, U = DQ_U, NW = DEC_NW;
  constexpr int US = (NR == 8 && U == 8) ? 2 : 4;  // key slots per softmax update
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
  const unsigned char* kb = p.k + (long)b * p.k_sb + (long)hk * p.k_sh + c * 8;
  const unsigned char* vb = p.v + (long)b * p.v_sb + (long)hk * p.v_sh + c * 8;
  const float* ksb = p.k_scale + (long)b * p.ks_sb + (long)hk * p.ks_sh;
  const float* vsb = p.v_scale + (long)b * p.vs_sb + (long)hk * p.vs_sh;

  auto load_tile = [&](int base, Fp8Tile& t) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * KPW + kg;
      t.k[u] = u32x2{0u, 0u};  // e4m3 0x00 is +0
      t.v[u] = u32x2{0u, 0u};
      t.ks[u] = 0.f;
      t.vs[u] = 0.f;
      if (key < k1) {
        ORION_DASSERT(key >= 0 && key < p.Tmax);
        t.k[u] = *reinterpret_cast<const u32x2*>(kb + (long)key * p.k_st);
        t.v[u] = *reinterpret_cast<const u32x2*>(vb + (long)key * p.v_st);
        t.ks[u] = ksb[key];
        t.vs[u] = vsb[key];
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
    Fp8Tile cur;
    if (base < k1) load_tile(base, cur);
    for (; base < k1; base += TILE) {
      Fp8Tile nxt = cur;
      if (base + TILE < k1) load_tile(base + TILE, nxt);  // next tile before this one's math

#pragma unroll
      for (int h = 0; h < U; h += US) {
        bf16x8 kc[US];
#pragma unroll
        for (int u = 0; u < US; ++u) kc[u] = fp8x8_to_bf16(cur.k[h + u][0], cur.k[h + u][1]);
        float pr[NR][US];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          float s[US];
          float mn = m[r];
#pragma unroll
          for (int u = 0; u < US; ++u) {
            const float d = key_lanes_sum<LPK>(dot8_bf16(qv[r], kc[u]));
            // select, not a zero weight: a stale key past the length must not reach the result
            s[u] = (base + (h + u) * KPW + kg < k1) ? d * cur.ks[h + u] * p.scale_log2 : -INFINITY;
            mn = fmaxf(mn, s[u]);
          }
          const float ms = finite_or_zero(mn);
          const float alpha = __builtin_amdgcn_exp2f(m[r] - ms);
          m[r] = mn;
          float ls = l[r] * alpha;
#pragma unroll
          for (int u = 0; u < US; ++u) {
            pr[r][u] = __builtin_amdgcn_exp2f(s[u] - ms);
            ls += pr[r][u];
          }
          l[r] = ls;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r][j] *= alpha;
        }
#pragma unroll
        for (int u = 0; u < US; ++u) {
          float vf[8];
          fp8x8_to_f32(cur.v[h + u][0], cur.v[h + u][1], vf);
#pragma unroll
          for (int r = 0; r < NR; ++r) {
            const float pv = pr[r][u] * cur.vs[h + u];  // the value scale folds into the weight
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[r][j] = fmaf(pv, vf[j], acc[r][j]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);  // one sub-block's conversions and weights live at a time
      }
      cur = nxt;
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

template <int D>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const AppendFp8Params p) {
  constexpr int P8 = D / 16;        // groups of 8 rotation pairs per head: the lanes of a head row
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
    const bool is_q = h < p.Hq;
    const int hh = is_q ? 0 : (h - p.Hq) % p.Hkv;
    const bool is_k = !is_q && h - p.Hq < p.Hkv;
    const bf16_t* src;
    if (is_q) {
      src = p.q + b * p.q_sb + t * p.q_st + h * p.q_sh;
      if (!ok) {  // no position to rotate at: a defined value for the skipped token
        bf16_t* dst = p.q_out + (((long)b * p.T + t) * p.Hq + h) * D;
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<bf16x8*>(dst + pg * 8) = z;
        *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = z;
        continue;
      }
    } else {
      if (!ok) continue;  // never written
      src = is_k ? p.k_new + b * p.kn_sb + t * p.kn_st + hh * p.kn_sh
                 : p.v_new + b * p.vn_sb + t * p.vn_st + hh * p.vn_sh;
    }
    const bf16x8 lo = *reinterpret_cast<const bf16x8*>(src + pg * 8);
    const bf16x8 hi = *reinterpret_cast<const bf16x8*>(src + D / 2 + pg * 8);
    float y1[8], y2[8];
    if (p.cosv != nullptr && (is_q || is_k)) {
      ORION_DASSERT(pos < p.npos);
      const float* cr = p.cosv + pos * (D / 2) + pg * 8;
      const float* sr = p.sinv + pos * (D / 2) + pg * 8;
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(cr), c1 = *reinterpret_cast<const f32x4*>(cr + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(sr), s1 = *reinterpret_cast<const f32x4*>(sr + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float cc = j < 4 ? c0[j] : c1[j - 4];
        const float ss = j < 4 ? s0[j] : s1[j - 4];
        const float x1 = bf2f(lo[j]), x2 = bf2f(hi[j]);
        y1[j] = x1 * cc - x2 * ss;
        y2[j] = x2 * cc + x1 * ss;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        y1[j] = bf2f(lo[j]);
        y2[j] = bf2f(hi[j]);
      }
    }
    if (is_q) {
      bf16_t* dst = p.q_out + (((long)b * p.T + t) * p.Hq + h) * D;
      bf16x8 o1, o2;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o1[j] = f2bf(y1[j]);
        o2[j] = f2bf(y2[j]);
      }
      *reinterpret_cast<bf16x8*>(dst + pg * 8) = o1;
      *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = o2;
      continue;
    }
    // the head row's amax: this thread's 16 values, then the row's P8 adjacent lanes
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) a = fmaxf(a, fmaxf(fabsf(y1[j]), fabsf(y2[j])));
    a = lanes_max<P8>(a);
    const float s = a > 0.f ? a / E4M3_MAX : 1.f;
    float z1[8], z2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // the clamp before the convert: nothing is left to its saturation mode
      z1[j] = fminf(fmaxf(y1[j] / s, -E4M3_MAX), E4M3_MAX);
      z2[j] = fminf(fmaxf(y2[j] / s, -E4M3_MAX), E4M3_MAX);
    }
    const u32x2 b1 = {f32x4_to_fp8(z1[0], z1[1], z1[2], z1[3]), f32x4_to_fp8(z1[4], z1[5], z1[6], z1[7])};
    const u32x2 b2 = {f32x4_to_fp8(z2[0], z2[1], z2[2], z2[3]), f32x4_to_fp8(z2[4], z2[5], z2[6], z2[7])};
    unsigned char* dst = is_k ? p.k_cache + b * p.kc_sb + pos * p.kc_st + hh * p.kc_sh
                              : p.v_cache + b * p.vc_sb + pos * p.vc_st + hh * p.vc_sh;
    ORION_DASSERT(hh < p.Hkv && b < p.B);
    *reinterpret_cast<u32x2*>(dst + pg * 8) = b1;
    *reinterpret_cast<u32x2*>(dst + D / 2 + pg * 8) = b2;
    if (pg == 0) {
      float* sc = is_k ? p.k_scale + b * p.ks_sb + hh * p.ks_sh : p.v_scale + b * p.vs_sb + hh * p.vs_sh;
      sc[pos] = s;
    }
  }
}

}  // namespace orion

using namespace orion;

int orion_attn_decode_fp8_tile(int D) { return D == 64 ? DecodeFp8Shape<64>::TILE : DecodeFp8Shape<128>::TILE; }

// orion_attn_decode_plan's rule on this kernel's key tile.
int orion_attn_decode_fp8_plan(int B, int Hkv, int Tmax, int D, int splits, int* chunk) {
  return orion_attn_decode_split_plan(orion_attn_decode_fp8_tile(D), B, Hkv, Tmax, splits, chunk);
}

template <int D>
static int launch_decode_fp8(const DecodeFp8Params& p, hipStream_t st) {
  const int G = p.Hq / p.Hkv;
  const dim3 grid(p.splits, p.Hkv, p.B);
  if (G > 4) attn_decode_fp8_kernel<D, 8><<<grid, 256, 0, st>>>(p);
  else if (G > 2) attn_decode_fp8_kernel<D, 4><<<grid, 256, 0, st>>>(p);
  else if (G == 2) attn_decode_fp8_kernel<D, 2><<<grid, 256, 0, st>>>(p);
  else attn_decode_fp8_kernel<D, 1><<<grid, 256, 0, st>>>(p);
  int rc = (int)hipGetLastError();
  if (rc || p.splits == 1) return rc;
  return orion_attn_decode_combine(p.ws_o, p.ws_ml, p.o, p.splits, D, (long)p.B * p.Hq, st);
}

int orion_attn_decode_fp8(const DecodeFp8Params& p, int D, hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (p.B <= 0 || p.Hkv <= 0 || p.Hq % p.Hkv || p.splits < 1 || p.chunk < 1) return -2;
  if (p.Hkv > 65535 || p.B > 65535) return -3;
  if (p.splits > 1 && (!p.ws_o || !p.ws_ml)) return -4;
  if ((long)p.splits * p.chunk > (1L << 30)) return -5;
  if (!p.k_scale || !p.v_scale) return -6;
  return D == 64 ? launch_decode_fp8<64>(p, st) : launch_decode_fp8<128>(p, st);
}

int orion_kv_append_fp8(const AppendFp8Params& p, hipStream_t st) {
  if (p.D != 64 && p.D != 128) return -1;
  if ((p.cosv == nullptr) != (p.sinv == nullptr)) return -2;
  if (p.Hq > 0 && (!p.q || !p.q_out || !p.cosv)) return -3;
  if (!p.k_scale || !p.v_scale) return -6;
  const long n = (long)p.B * p.T * (p.Hq + 2 * p.Hkv) * (p.D / 16);
  if (n <= 0) return 0;
  long g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  if (p.D == 64) kv_append_fp8_kernel<64><<<(int)g, 256, 0, st>>>(p);
  else kv_append_fp8_kernel<128><<<(int)g, 256, 0, st>>>(p);
  return (int)hipGetLastError();
}
