// Parameter block shared by csrc/linear_decode_mxfp4.hip and csrc/bindings.cpp.
#pragma once

#include "linear_decode_params.h"  // LinearDecodeNorm, LinearDecodeAct

namespace orion {

// y[M, Nout] = epi(pro(x)[M, K] . W[N, K]^T) for 1 <= M <= 16 (linear_decode_mxfp4_kernel): the
// weight is OCP MXFP4, W[n, k] = 2^(w_scale[n][k / 32] - 127) e2m1(code[n][k]), two codes per byte
// of wq (even k in the low nibble).  N = Nout, or 2 Nout with LD_ACT_SWIGLU (rows [0, Nout) the
// gate, [Nout, 2 Nout) the up half).
struct LinearDecodeMxfp4Params {
  const unsigned short* x;       // (M, K) bf16 bits, unit stride on K, row stride x_rs
  const unsigned char* wq;       // (N, K / 2) code pairs, contiguous, K % 32 == 0
  const unsigned char* w_scale;  // (N, K / 32) e8m0, contiguous
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
