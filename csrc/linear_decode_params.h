// Parameter block shared by csrc/linear_decode.hip and csrc/bindings.cpp.
#pragma once

namespace orion {

enum LinearDecodeNorm { LD_NORM_NONE = 0, LD_NORM_LAYER = 1, LD_NORM_RMS = 2 };
enum LinearDecodeAct { LD_ACT_NONE = 0, LD_ACT_GELU = 1, LD_ACT_SWIGLU = 2 };

// y[M, Nout] = epi(pro(x)[M, K] . W[N, K]^T) for 1 <= M <= 16 (linear_decode_kernel).
// N = Nout, or 2 Nout with LD_ACT_SWIGLU (rows [0, Nout) the gate, [Nout, 2 Nout) the up half).
struct LinearDecodeParams {
  const unsigned short* x;       // (M, K) bf16 bits, unit stride on K, row stride x_rs
  const unsigned short* w;       // (N, K) contiguous
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
