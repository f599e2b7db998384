// Parameter block shared by csrc/linear_decode_fp8.hip and csrc/bindings.cpp.
#pragma once

#include "linear_decode_params.h"  // LinearDecodeNorm, LinearDecodeAct

namespace orion {

// y[M, Nout] = epi(scale . (pro(x)[M, K] . Q[N, K]^T)) for 1 <= M <= 16 (linear_decode_fp8_kernel):
// the weight is OCP e4m3fn bytes Q with one fp32 scale per row, W[n, k] = scale[n] Q[n, k].
// N = Nout, or 2 Nout with LD_ACT_SWIGLU (rows [0, Nout) the gate, [Nout, 2 Nout) the up half).
struct LinearDecodeFp8Params {
  const unsigned short* x;       // (M, K) bf16 bits, unit stride on K, row stride x_rs
  const unsigned char* wq;       // (N, K) e4m3fn, contiguous, K % 16 == 0
  const float* w_scale;          // (N,)
  const unsigned short* bias;    // (N,) or null
  const unsigned short* norm_w;  // (K,) gamma, null without a prologue
  const unsigned short* norm_b;  // (K,) beta or null (LayerNorm only)
  const unsigned short* res;     // (M, Nout) residual stream, row stride res_rs, or null
  unsigned short* y;             // (M, Nout), row stride y_rs
  long x_rs, res_rs, y_rs;
  int M, K, Nout;
  int norm, act;
  float eps;
};

}  // namespace orion
