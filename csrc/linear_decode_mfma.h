// Device helpers shared by csrc/linear_decode.hip, csrc/linear_decode_fp8.hip and
// csrc/linear_decode_mxfp4.hip.
#pragma once

#include "common.h"

namespace orion {

ORION_DEVICE f32x4 ld_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_mfma, a),
                                                 __builtin_bit_cast(bf16x8_mfma, b), c, 0, 0, 0);
}

ORION_DEVICE float sum16(float v) {  // over the aligned group of 16 lanes, every lane the total
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace orion
