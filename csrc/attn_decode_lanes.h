// Lane-level helpers of the decode attention kernel (csrc/attn_decode_core.h) and the cache appends
// (csrc/attn_decode.hip), on a bf16 or an FP8 cache: a key row of D elements is spread 8 elements per
// lane over an aligned group of D / 8 = 8 or 16 lanes.
#pragma once

#include "common.h"

namespace orion {

constexpr int DEC_NW = 4;  // waves per workgroup

// 8 bf16 products summed in fp32: four v_dot2c_f32_bf16.  The pairs are taken by shufflevector
// on the __bf16 vector: taking them as words of a u32x4 bit cast compiled to four dots of word 0.
ORION_DEVICE float dot8_bf16(bf16x8 a, bf16x8 b) {
  const bf16x8_mfma av = __builtin_bit_cast(bf16x8_mfma, a), bv = __builtin_bit_cast(bf16x8_mfma, b);
  float s = 0.f;
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 0, 1), __builtin_shufflevector(bv, bv, 0, 1),
                                      s, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 2, 3), __builtin_shufflevector(bv, bv, 2, 3),
                                      s, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 4, 5), __builtin_shufflevector(bv, bv, 4, 5),
                                      s, false);
  s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(av, av, 6, 7), __builtin_shufflevector(bv, bv, 6, 7),
                                      s, false);
  return s;
}

// v and the v of another lane of its row of 16, by a DPP move (no LDS-pipe ds_bpermute)
template <int CTRL>
ORION_DEVICE float dpp_move(float v) {
  const int x = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false));
}

template <int CTRL>
ORION_DEVICE float dpp_add(float v) { return v + dpp_move<CTRL>(v); }

template <int CTRL>
ORION_DEVICE float dpp_max(float v) { return fmaxf(v, dpp_move<CTRL>(v)); }

// Sum over the aligned group of LPK (8 or 16) lanes that hold one key row, every lane getting
// the total, on DPP moves: quad_perm [1,0,3,2] and [2,3,0,1] sum a quad; the quads' sums being
// uniform, row_half_mirror (lane i <- 7 - i) adds the other quad of the 8 and row_mirror
// (i <- 15 - i) the other half of the 16-lane row.
template <int LPK>
ORION_DEVICE float key_lanes_sum(float v) {
  static_assert(LPK == 8 || LPK == 16, "a key row spans 8 or 16 lanes");
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  if constexpr (LPK == 16) v = dpp_add<0x140>(v);  // row_mirror
  return v;
}

// The same walk with max over an aligned group of 4 or 8 lanes (the append's amax of a head row).
template <int LANES>
ORION_DEVICE float lanes_max(float v) {
  static_assert(LANES == 4 || LANES == 8, "a head row spans 4 or 8 lanes");
  v = dpp_max<0xB1>(v);
  v = dpp_max<0x4E>(v);
  if constexpr (LANES == 8) v = dpp_max<0x141>(v);
  return v;
}

ORION_DEVICE float finite_or_zero(float m) { return m == -INFINITY ? 0.f : m; }

// The cache appends' thread mapping: element i is group pg of 8 rotation pairs (the lower and the
// upper 8 elements at pg * 8 and D / 2 + pg * 8) of head h, among the HT = Hq + 2 Hkv heads
// q | k_new | v_new of token t of row b; the token lands at pos, and is skipped when !ok.
struct AppendIndex {
  int pg, h, t, b;
  long pos;
  bool ok;
};

ORION_DEVICE AppendIndex append_index(long i, int P8, int HT, int T, const int* kv_lens, int Tmax) {
  AppendIndex x;
  x.pg = (int)(i % P8);
  const long row = i / P8;
  x.h = (int)(row % HT);
  x.t = (int)((row / HT) % T);
  x.b = (int)(row / ((long)HT * T));
  x.pos = (long)kv_lens[x.b] + x.t;
  x.ok = x.pos >= 0 && x.pos < Tmax;
  return x;
}

// A skipped token has no position to rotate at: its q row gets a defined value.
ORION_DEVICE void append_zero_q(bf16_t* dst, int D, int pg) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  *reinterpret_cast<bf16x8*>(dst + pg * 8) = z;
  *reinterpret_cast<bf16x8*>(dst + D / 2 + pg * 8) = z;
}

// The 8 pairs (lo[j], hi[j]) rotated in fp32 by row pos of the [npos][D / 2] tables; not rounded.
ORION_DEVICE void rotate_pairs(const float* cosv, const float* sinv, long pos, int D, int pg, bf16x8 lo, bf16x8 hi,
                               float (&y1)[8], float (&y2)[8]) {
  const float* cr = cosv + pos * (D / 2) + pg * 8;
  const float* sr = sinv + pos * (D / 2) + pg * 8;
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
}

}  // namespace orion
