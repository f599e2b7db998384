// Multi-query decode attention for gfx950 (wave64, bf16 in, fp32 math): Tq <= 16 queries per row
// against a key/value cache with a causal tail, for a verify step of speculative decoding.
//
// attn_decode_multi_kernel<D, NR>, grid (splits, Hkv, B), 256 threads: attn_decode_kernel
// (csrc/attn_decode.hip) with the workgroup's rows being the Tq * G pairs (t, g) of its KV head,
// G = Hq / Hkv, t-major, NR <= 8 at a time.  The lane geometry, the key tiles, the loads (16
// bytes per lane straight to VGPRs, the next tile's issued before this tile's math), the base-2
// online softmax per (wave, key slot), the merge order and the combine kernel are that kernel's.
// The one per-row difference is the key bound in the score select: query t of row b sees keys
// [0, lim_t), lim_t = clamp(kv_lens[b] - Tq + 1 + t, 0, min(kv_lens[b], Tmax)), and the tile loop
// of a pass runs to the largest bound among its rows.
//
// Row (b, t) equals, bit for bit, attn_decode_kernel on kv_lens[b] - (Tq - 1 - t) with the same
// split plan: within its bound a row sees the same scores in the same tiles; a key at or past its
// bound has score -inf by select, weight 2^(-inf) = 0, and fma(0, v, acc) = acc for the finite v
// of a valid key; a tile wholly past the bound has alpha = 2^(m - m) = 1 (or keeps the neutral
// (-inf, 0, 0): alpha = 2^(-inf - 0) = 0 on l = 0, acc = 0), so m, l and acc do not change.
// Keys at or beyond min(kv_lens[b], Tmax) are never loaded.
#include "common.h"
#include "attn_decode_lanes.h"
#include "launchers.h"

namespace orion {

namespace {

constexpr int DECM_U = 4;  // K (and V) loads in flight per wave and tile: attn_decode_kernel's

template <int D>
struct DecodeMultiShape {
  static constexpr int LPK = D / 8;                   // lanes per key row
  static constexpr int KPW = 64 / LPK;                // keys per wave-wide load
  static constexpr int TILE = DEC_NW * DECM_U * KPW;  // keys per workgroup iteration
};

}  // namespace

template <int D, int NR>
__global__ __launch_bounds__(256) void attn_decode_multi_kernel(const DecodeMultiParams p) {
  typedef DecodeMultiShape<D> S;
  constexpr int LPK = S::LPK, KPW = S::KPW, TILE = S::TILE, U = DECM_U, NW = DEC_NW;
  __shared__ float sm[NW][NR][D + 2];  // per wave and row: o[D], m, l

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane % LPK, kg = lane / LPK;
  const int G = p.Hq / p.Hkv, R = p.Tq * G;
  ORION_DASSERT(b < p.B && hk < p.Hkv && split < p.splits);

  const int kvl = p.kv_lens[b];
  const int len = kvl < 0 ? 0 : (kvl > p.Tmax ? p.Tmax : kvl);
  const long first = (long)kvl - p.Tq + 1;  // query 0's bound before the clamp
  const int k0 = split * p.chunk;
  // the keys of this split that query t sees end at bound(t); <= k0: none
  auto bound = [&](int t) {
    const long lim = first + t;
    const int l = lim < 0 ? 0 : (lim > len ? len : (int)lim);
    return min(k0 + p.chunk, l);
  };
  const bf16_t* kb = p.k + (long)b * p.k_sb + (long)hk * p.k_sh + c * 8;
  const bf16_t* vb = p.v + (long)b * p.v_sb + (long)hk * p.v_sh + c * 8;

  for (int r0 = 0; r0 < R; r0 += NR) {
    const int k1 = bound((min(r0 + NR, R) - 1) / G);  // the pass's largest bound: t-major rows

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

    bf16x8 qv[NR];
    int kr[NR];  // each row's own key bound (workgroup-uniform)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      qv[r] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      kr[r] = 0;
      if (r0 + r < R) {
        const int t = (r0 + r) / G, hq = hk * G + (r0 + r) % G;
        ORION_DASSERT(t < p.Tq && hq < p.Hq);
        kr[r] = bound(t);
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
          // select, not a zero weight: the row's causal bound and the stale keys past the length
          s[u] = (base + u * KPW + kg < kr[r]) ? d * p.scale_log2 : -INFINITY;
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
      const int t = (r0 + r) / G, hq = hk * G + (r0 + r) % G;
      const long head = ((long)b * p.Tq + t) * p.Hq + hq;  // (b, t, head) flattened
      ORION_DASSERT(head < (long)p.B * p.Tq * p.Hq);
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

using namespace orion;

template <int D>
static int launch_decode_multi(const DecodeMultiParams& p, hipStream_t st) {
  if (p.chunk % DecodeMultiShape<D>::TILE) return -2;  // the split plan is the single-query kernel's
  const int R = p.Tq * (p.Hq / p.Hkv);
  const dim3 grid(p.splits, p.Hkv, p.B);
  if (R > 4) attn_decode_multi_kernel<D, 8><<<grid, 256, 0, st>>>(p);
  else if (R > 2) attn_decode_multi_kernel<D, 4><<<grid, 256, 0, st>>>(p);
  else if (R == 2) attn_decode_multi_kernel<D, 2><<<grid, 256, 0, st>>>(p);
  else attn_decode_multi_kernel<D, 1><<<grid, 256, 0, st>>>(p);
  int rc = (int)hipGetLastError();
  if (rc || p.splits == 1) return rc;
  return orion_attn_decode_combine(p.ws_o, p.ws_ml, p.o, p.splits, D, (long)p.B * p.Tq * p.Hq, st);
}

int orion_attn_decode_multi(const DecodeMultiParams& p, int D, hipStream_t st) {
  if (D != 64 && D != 128) return -1;
  if (p.B <= 0 || p.Hkv <= 0 || p.Hq % p.Hkv || p.splits < 1 || p.chunk < 1) return -2;
  if (p.Tq < 1 || p.Tq > 16) return -2;
  if (p.Hkv > 65535 || p.B > 65535) return -3;
  if (p.splits > 1 && (!p.ws_o || !p.ws_ml)) return -4;
  if ((long)p.splits * p.chunk > (1L << 30)) return -5;
  return D == 64 ? launch_decode_multi<64>(p, st) : launch_decode_multi<128>(p, st);
}
