// The decode attention kernel of csrc/attn_decode.hip for gfx950 (wave64, bf16 q and o, fp32 math):
// attention of a few queries per row over a key/value cache, split over keys.  One body,
// attn_decode_kernel<D, NR, FP8, MULTI>, instantiated for a bf16 or an FP8 cache (FP8) and for one
// query per row or Tq <= 16 with a causal tail (MULTI); both switches are compile-time, so nothing
// of the other form is left in an instantiation.  Device code only.
//
// Grid (splits, Hkv, B), 256 threads:
//   * decode is a memory-bound stream of K and V, so one workgroup serves all G = Hq / Hkv query
//     heads of its KV head (K / V leave memory once per KV head, not once per query head), NR <= 8
//     rows at a time (the rows are looped when there are more than 8: a later pass hits the L2);
//   * a key row is D elements = D / 8 lanes of one load each, so a wave's load instruction
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
// FP8 (OCP e4m3fn bytes with one fp32 scale per (row, KV head, token); value = scale * byte): a
// lane's load is 8 bytes, half the bf16 cache's, at the same U = 4, so the tile, the register budget
// and the waves per SIMD are the bf16 kernel's.  K bytes become packed bf16
// (v_cvt_scalef32_pk_bf16_fp8 at scale 1, exact) for the same dot against the packed q, V bytes fp32
// (v_cvt_pk_f32_fp8, exact).  The scales are plain fp32 multiplies: score = (q . k_bytes)
// k_scale[key] scale_log2, and the value scale folds into the weight: acc += (p v_scale[key])
// v_bytes, l += p.  The scales of a key are one load per lane (the D / 8 lanes of a key read one
// address; a wave's keys are consecutive floats), loaded like the bytes only below the length: a
// stale 0x7F byte or NaN scale beyond it cannot reach the result.  With unit scales the result is
// the bf16 kernel's on the widened cache, bit for bit.  U = 8 (the bf16 cache's bytes in flight per
// wave) was measured and not kept: docs/PERFORMANCE.md "FP8 KV cache" and
// profiles/decode/kernel_resources_attn_decode_fp8.txt; what this kernel gains from is waves per
// SIMD, not bytes in flight per wave.
//
// MULTI (a verify step of speculative decoding): the workgroup's rows are the Tq * G pairs (t, g)
// of its KV head, t-major.  The one per-row difference is the key bound in the score select: query t
// of row b sees keys [0, lim_t), lim_t = clamp(kv_lens[b] - Tq + 1 + t, 0, min(kv_lens[b], Tmax)),
// and the tile loop of a pass runs to the largest bound among its rows.  Row (b, t) equals, bit for
// bit, the single-query instantiation on kv_lens[b] - (Tq - 1 - t) with the same split plan: within
// its bound a row sees the same scores in the same tiles; a key at or past its bound has score -inf
// by select, weight 2^(-inf) = 0, and fma(0, v, acc) = acc for the finite v of a valid key; a tile
// wholly past the bound has alpha = 2^(m - m) = 1 (or keeps the neutral (-inf, 0, 0): alpha =
// 2^(-inf - 0) = 0 on l = 0, acc = 0), so m, l and acc do not change.  The single-query
// instantiation keeps no per-row bounds.
//
// <D, NR, true, true> is not instantiated: multi-query over an FP8 cache is one more line in
// csrc/attn_decode.hip's launcher, plus its binding.
#pragma once

#include <type_traits>

#include "common.h"
#include "attn_decode_lanes.h"
#include "attn_decode_params.h"
#include "fp8_cvt.h"

namespace orion {

constexpr int DEC_U = 4;  // K (and V) loads in flight per wave and tile

template <int D>
struct DecodeShape {
  static constexpr int LPK = D / 8;                  // lanes per key row
  static constexpr int KPW = 64 / LPK;               // keys per wave-wide load
  static constexpr int TILE = DEC_NW * DEC_U * KPW;  // keys per workgroup iteration
};

// One wave's share of a key tile in registers: 8 elements of K and of V per lane and key slot.
template <bool FP8>
struct DecodeTile {
  bf16x8 k[DEC_U], v[DEC_U];
};
template <>
struct DecodeTile<true> {
  u32x2 k[DEC_U], v[DEC_U];
  float ks[DEC_U], vs[DEC_U];
};

template <int D, int NR, bool FP8, bool MULTI>
__global__ __launch_bounds__(256) void attn_decode_kernel(const DecodeParams p) {
  typedef DecodeShape<D> S;
  typedef typename std::conditional<FP8, unsigned char, bf16_t>::type elem_t;
  typedef typename std::conditional<FP8, u32x2, bf16x8>::type load_t;
  constexpr int LPK = S::LPK, KPW = S::KPW, TILE = S::TILE, U = DEC_U, NW = DEC_NW;
  __shared__ float sm[NW][NR][D + 2];  // per wave and row: o[D], m, l

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane % LPK, kg = lane / LPK;
  const int G = p.Hq / p.Hkv, Tq = MULTI ? p.Tq : 1, R = Tq * G;
  ORION_DASSERT(b < p.B && hk < p.Hkv && split < p.splits);

  const int kvl = p.kv_lens[b];
  const int len = kvl < 0 ? 0 : (kvl > p.Tmax ? p.Tmax : kvl);
  const long first = (long)kvl - Tq + 1;  // MULTI: query 0's bound before the clamp
  const int k0 = split * p.chunk;
  // the keys of this split that query t sees end at bound(t); <= k0: none
  auto bound = [&](int t) {
    if constexpr (MULTI) {
      const long lim = first + t;
      const int l = lim < 0 ? 0 : (lim > len ? len : (int)lim);
      return min(k0 + p.chunk, l);
    } else {
      return min(k0 + p.chunk, len);
    }
  };
  const elem_t* kb = (const elem_t*)p.k + (long)b * p.k_sb + (long)hk * p.k_sh + c * 8;
  const elem_t* vb = (const elem_t*)p.v + (long)b * p.v_sb + (long)hk * p.v_sh + c * 8;
  const float* ksb = FP8 ? p.k_scale + (long)b * p.ks_sb + (long)hk * p.ks_sh : nullptr;
  const float* vsb = FP8 ? p.v_scale + (long)b * p.vs_sb + (long)hk * p.vs_sh : nullptr;

  for (int r0 = 0; r0 < R; r0 += NR) {
    // the keys of this pass: MULTI, its largest bound (the rows are t-major)
    const int k1 = bound(MULTI ? (min(r0 + NR, R) - 1) / G : 0);

    auto load_tile = [&](int base, DecodeTile<FP8>& t) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int key = base + u * KPW + kg;
        t.k[u] = load_t{};  // e4m3 0x00 is +0
        t.v[u] = load_t{};
        if constexpr (FP8) {
          t.ks[u] = 0.f;
          t.vs[u] = 0.f;
        }
        if (key < k1) {
          ORION_DASSERT(key >= 0 && key < p.Tmax);
          t.k[u] = *reinterpret_cast<const load_t*>(kb + (long)key * p.k_st);
          t.v[u] = *reinterpret_cast<const load_t*>(vb + (long)key * p.v_st);
          if constexpr (FP8) {
            t.ks[u] = ksb[key];
            t.vs[u] = vsb[key];
          }
        }
      }
    };

    bf16x8 qv[NR];
    int kr[MULTI ? NR : 1];  // MULTI: each row's own key bound (workgroup-uniform)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      qv[r] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if constexpr (MULTI) kr[r] = 0;
      if (r0 + r < R) {
        const int t = MULTI ? (r0 + r) / G : 0, hq = hk * G + (MULTI ? (r0 + r) % G : r0 + r);
        ORION_DASSERT(t < Tq && hq < p.Hq);
        if constexpr (MULTI) kr[r] = bound(t);
        qv[r] = *reinterpret_cast<const bf16x8*>(p.q + (long)b * p.q_sb + (long)t * p.q_st + (long)hq * p.q_sh +
                                                 c * 8);
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
    DecodeTile<FP8> cur;
    if (base < k1) load_tile(base, cur);
    for (; base < k1; base += TILE) {
      DecodeTile<FP8> nxt = cur;
      if (base + TILE < k1) load_tile(base + TILE, nxt);  // next tile before this one's math

      bf16x8 kc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (FP8) kc[u] = fp8x8_to_bf16(cur.k[u][0], cur.k[u][1]);
        else kc[u] = cur.k[u];
      }
      float pr[NR][U];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int kend = MULTI ? kr[r] : k1;
        float s[U];
        float mn = m[r];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float d = key_lanes_sum<LPK>(dot8_bf16(qv[r], kc[u]));
          if constexpr (FP8) d *= cur.ks[u];
          // select, not a zero weight: a key past the row's bound or the length must not reach the result
          s[u] = (base + u * KPW + kg < kend) ? d * p.scale_log2 : -INFINITY;
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
        if constexpr (FP8) {
          fp8x8_to_f32(cur.v[u][0], cur.v[u][1], vf);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) vf[j] = bf2f(cur.v[u][j]);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          float pv = pr[r][u];
          if constexpr (FP8) pv *= cur.vs[u];  // the value scale folds into the weight
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r][j] = fmaf(pv, vf[j], acc[r][j]);
        }
      }
      // FP8: this tile's conversions and weights are dead before the next tile's are made
      if constexpr (FP8) __builtin_amdgcn_sched_barrier(0);
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
      if (r0 + r >= R) continue;
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
      const int t = MULTI ? (r0 + r) / G : 0, hq = hk * G + (MULTI ? (r0 + r) % G : r0 + r);
      const long head = ((long)b * Tq + t) * p.Hq + hq;  // (b, t, head) flattened
      ORION_DASSERT(head < (long)p.B * Tq * p.Hq);
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
    __syncthreads();  // sm is reused by the next pass
  }
}

}  // namespace orion
