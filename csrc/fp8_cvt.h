// OCP e4m3fn bytes <-> bf16 / fp32 in registers on gfx950, shared by csrc/linear_decode_fp8.hip and
// csrc/attn_decode_core.h.  Every e4m3 value is a bf16 (and an fp32) value, so the widening
// conversions are exact; the narrowing one rounds to nearest even and is only given values
// already clamped to [-448, 448].
#pragma once

#include "common.h"

namespace orion {

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;  // 8 e4m3 bytes

constexpr float E4M3_MAX = 448.f;  // the largest finite e4m3fn value

// 8 e4m3 bytes (two words, ascending index) -> 8 bf16: v_cvt_scalef32_pk_bf16_fp8 at scale 1,
// two bytes of a word per instruction
ORION_DEVICE bf16x8 fp8x8_to_bf16(unsigned w0, unsigned w1) {
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w0, 1.0f, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w1, 1.0f, true));
  return __builtin_bit_cast(bf16x8, r);
}

// 8 e4m3 bytes -> 8 fp32 (v_cvt_pk_f32_fp8: the low or the high two bytes of a word)
ORION_DEVICE void fp8x8_to_f32(unsigned w0, unsigned w1, float (&f)[8]) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
  f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
}

// 4 fp32 in [-448, 448] -> one word of 4 e4m3 bytes, ascending index (v_cvt_pk_fp8_f32, RNE)
ORION_DEVICE unsigned f32x4_to_fp8(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}

}  // namespace orion
