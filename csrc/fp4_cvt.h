// OCP MXFP4 (e2m1 codes, one e8m0 scale per 32) -> bf16 in registers on gfx950, used by
// csrc/linear_decode_mxfp4.hip.  A code is sign, two exponent bits, one mantissa bit: magnitudes
// 0, 0.5, 1, 1.5, 2, 3, 4, 6.  Storage order (orion_amd/ops/mxfp4.py): even k in the low nibble of
// a byte, odd k in the high one, bytes ascending in k.
#pragma once

#include "common.h"

namespace orion {

// The fp32 2^(byte - 127) of an e8m0 scale byte in [1, 254]: the byte is the exponent field.
ORION_DEVICE float e8m0_to_f32(unsigned byte) { return __builtin_bit_cast(float, byte << 23); }

// 8 e2m1 codes (one word, ascending k) times `scale` -> 8 bf16: v_cvt_scalef32_pk_bf16_fp4, one
// byte of the word per instruction (op_sel 0..3), its low nibble into the low half of the result.
// Exact whenever code x scale is a normal bf16: an e2m1 value has a 2-bit significand, and the
// scale is a power of two.
ORION_DEVICE bf16x8 fp4x8_to_bf16(unsigned w, float scale) {
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return __builtin_bit_cast(bf16x8, r);
}

}  // namespace orion
