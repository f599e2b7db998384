// Generation-time attention for gfx950 over a bf16 or an FP8 (OCP e4m3fn) key/value cache: the
// instantiations and the launcher of csrc/attn_decode_core.h's attn_decode_kernel (read its header
// for the design), the merge of its splits' partials, the split plan, and the two cache appends
// (optionally with RoPE).
//
// kv_append_kernel: one thread per 8 rotation pairs (two 16-byte loads and stores) of a head
// of q | k_new | v_new; k (rotated in fp32 at position kv_lens[b] + t when tables are given,
// rounded once) and v (copied bit for bit) land in the cache, the rotated q in a contiguous
// output.  Positions outside [0, Tmax) are skipped (their q rows are zero).
//
// kv_append_fp8_kernel<D>: the same thread mapping; the quantisation rule is orion_amd/ops/fp8.py's
// quantize_kv_fp8.  q is rotated and stored as bf16 exactly as there.  k (rotated in fp32, not
// rounded to bf16) and v: amax over the thread's 16 values and, by DPP moves, over the D / 16
// adjacent lanes of the head row; scale = amax / 448 (1 for a zero row; an IEEE division); byte =
// e4m3(clamp(x / scale, -448, 448)), the clamp before v_cvt_pk_fp8_f32; two 8-byte stores, and lane
// 0 of the row stores the scale.  The D / 16 lanes of a row are adjacent, all inside the loop and all
// on the same branch together: the element count and the grid stride are multiples of D / 16 and the
// branches depend on the row only.
#include "attn_decode_core.h"
#include "launchers.h"

namespace orion {

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
    const AppendIndex x = append_index(i, P8, HT, p.T, p.kv_lens, p.Tmax);
    const int pg = x.pg, h = x.h, t = x.t, b = x.b;
    const long pos = x.pos;
    const bf16_t* src;
    bf16_t* dst;
    bool rot = p.cosv != nullptr;
    if (h < p.Hq) {
      src = p.q + b * p.q_sb + t * p.q_st + h * p.q_sh;
      dst = p.q_out + (((long)b * p.T + t) * p.Hq + h) * D;
      if (!x.ok) {
        append_zero_q(dst, D, pg);
        continue;
      }
    } else {
      if (!x.ok) continue;  // never written
      const int hh = h - p.Hq;
      if (hh < p.Hkv) {
        src = p.k_new + b * p.kn_sb + t * p.kn_st + hh * p.kn_sh;
        dst = (bf16_t*)p.k_cache + b * p.kc_sb + pos * p.kc_st + hh * p.kc_sh;
      } else {
        src = p.v_new + b * p.vn_sb + t * p.vn_st + (hh - p.Hkv) * p.vn_sh;
        dst = (bf16_t*)p.v_cache + b * p.vc_sb + pos * p.vc_st + (hh - p.Hkv) * p.vc_sh;
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
    float y1[8], y2[8];
    rotate_pairs(p.cosv, p.sinv, pos, D, pg, lo, hi, y1, y2);
    bf16x8 o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o1[j] = f2bf(y1[j]);
      o2[j] = f2bf(y2[j]);
    }
    *reinterpret_cast<bf16x8*>(dst + pg * 8) = o1;
    *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = o2;
  }
}

template <int D>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const AppendParams p) {
  constexpr int P8 = D / 16;        // groups of 8 rotation pairs per head: the lanes of a head row
  const int HT = p.Hq + 2 * p.Hkv;  // heads per token: q | k | v (p.Hq = 0 without q)
  const long n = (long)p.B * p.T * HT * P8;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const AppendIndex x = append_index(i, P8, HT, p.T, p.kv_lens, p.Tmax);
    const int pg = x.pg, h = x.h, t = x.t, b = x.b;
    const long pos = x.pos;
    const bool is_q = h < p.Hq;
    const int hh = is_q ? 0 : (h - p.Hq) % p.Hkv;
    const bool is_k = !is_q && h - p.Hq < p.Hkv;
    const bf16_t* src;
    if (is_q) {
      src = p.q + b * p.q_sb + t * p.q_st + h * p.q_sh;
      if (!x.ok) {
        append_zero_q(p.q_out + (((long)b * p.T + t) * p.Hq + h) * D, D, pg);
        continue;
      }
    } else {
      if (!x.ok) continue;  // never written
      src = is_k ? p.k_new + b * p.kn_sb + t * p.kn_st + hh * p.kn_sh
                 : p.v_new + b * p.vn_sb + t * p.vn_st + hh * p.vn_sh;
    }
    const bf16x8 lo = *reinterpret_cast<const bf16x8*>(src + pg * 8);
    const bf16x8 hi = *reinterpret_cast<const bf16x8*>(src + D / 2 + pg * 8);
    float y1[8], y2[8];
    if (p.cosv != nullptr && (is_q || is_k)) {
      ORION_DASSERT(pos < p.npos);
      rotate_pairs(p.cosv, p.sinv, pos, D, pg, lo, hi, y1, y2);
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
    unsigned char* dst = is_k ? (unsigned char*)p.k_cache + b * p.kc_sb + pos * p.kc_st + hh * p.kc_sh
                              : (unsigned char*)p.v_cache + b * p.vc_sb + pos * p.vc_st + hh * p.vc_sh;
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

// The kernel's key tile is the same on both cache types, so this is the plan of all three ops.
int orion_attn_decode_plan(int B, int Hkv, int Tmax, int D, int splits, int* chunk) {
  const int tile = D == 64 ? DecodeShape<64>::TILE : DecodeShape<128>::TILE;
  return orion_attn_decode_split_plan(tile, B, Hkv, Tmax, splits, chunk);
}

// The merge of the splits' partials into bf16 o (`heads` heads of D columns).
int orion_attn_decode_combine(const float* ws_o, const float* ws_ml, void* o, int splits, int D, long heads,
                              hipStream_t st) {
  const long n = heads * D;
  attn_decode_combine_kernel<<<(int)((n + 255) / 256), 256, 0, st>>>(ws_o, ws_ml, (bf16_t*)o, splits, D, heads);
  return (int)hipGetLastError();
}

template <int D, bool FP8, bool MULTI>
static int launch_decode(const DecodeParams& p, hipStream_t st) {
  if (MULTI && p.chunk % DecodeShape<D>::TILE) return -2;  // a row's bit-equality with a single query: whole tiles
  const int R = p.Tq * (p.Hq / p.Hkv);
  const dim3 grid(p.splits, p.Hkv, p.B);
  if (R > 4) attn_decode_kernel<D, 8, FP8, MULTI><<<grid, 256, 0, st>>>(p);
  else if (R > 2) attn_decode_kernel<D, 4, FP8, MULTI><<<grid, 256, 0, st>>>(p);
  else if (R == 2) attn_decode_kernel<D, 2, FP8, MULTI><<<grid, 256, 0, st>>>(p);
  else attn_decode_kernel<D, 1, FP8, MULTI><<<grid, 256, 0, st>>>(p);
  int rc = (int)hipGetLastError();
  if (rc || p.splits == 1) return rc;
  return orion_attn_decode_combine(p.ws_o, p.ws_ml, p.o, p.splits, D, (long)p.B * p.Tq * p.Hq, st);
}

template <bool FP8, bool MULTI>
static int decode(const DecodeParams& p, int D, hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (p.B <= 0 || p.Hkv <= 0 || p.Hq % p.Hkv || p.splits < 1 || p.chunk < 1) return -2;
  if (MULTI ? p.Tq < 1 || p.Tq > 16 : p.Tq != 1) return -2;
  if (p.Hkv > 65535 || p.B > 65535) return -3;
  if (p.splits > 1 && (!p.ws_o || !p.ws_ml)) return -4;
  if ((long)p.splits * p.chunk > (1L << 30)) return -5;
  if (FP8 && (!p.k_scale || !p.v_scale)) return -6;
  return D == 64 ? launch_decode<64, FP8, MULTI>(p, st) : launch_decode<128, FP8, MULTI>(p, st);
}

int orion_attn_decode(const DecodeParams& p, int D, hipStream_t st) { return decode<false, false>(p, D, st); }
int orion_attn_decode_fp8(const DecodeParams& p, int D, hipStream_t st) { return decode<true, false>(p, D, st); }
int orion_attn_decode_multi(const DecodeParams& p, int D, hipStream_t st) { return decode<false, true>(p, D, st); }

static int append_grid(const AppendParams& p) {
  const long n = (long)p.B * p.T * (p.Hq + 2 * p.Hkv) * (p.D / 16);
  const long g = (n + 255) / 256;
  return n <= 0 ? 0 : (int)(g > 4096 ? 4096 : g);
}

int orion_kv_append(const AppendParams& p, hipStream_t st) {
  if (p.D % 16) return -1;
  if ((p.cosv == nullptr) != (p.sinv == nullptr)) return -2;
  if (p.Hq > 0 && (!p.q || !p.q_out || !p.cosv)) return -3;
  const int g = append_grid(p);
  if (g == 0) return 0;
  kv_append_kernel<<<g, 256, 0, st>>>(p);
  return (int)hipGetLastError();
}

int orion_kv_append_fp8(const AppendParams& p, hipStream_t st) {
  if (p.D != 64 && p.D != 128) return -1;
  if ((p.cosv == nullptr) != (p.sinv == nullptr)) return -2;
  if (p.Hq > 0 && (!p.q || !p.q_out || !p.cosv)) return -3;
  if (!p.k_scale || !p.v_scale) return -6;
  const int g = append_grid(p);
  if (g == 0) return 0;
  if (p.D == 64) kv_append_fp8_kernel<64><<<g, 256, 0, st>>>(p);
  else kv_append_fp8_kernel<128><<<g, 256, 0, st>>>(p);
  return (int)hipGetLastError();
}
