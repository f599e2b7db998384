// Parameter block shared by csrc/sample.hip and csrc/bindings.cpp.
#pragma once

namespace orion {

// One token per row of logits (B, V) by the models' sampling rule (sample_kernel).  Everything a
// captured launch must see change from token to token is read from device memory.
struct SampleParams {
  const unsigned short* logits;  // (B, V) bf16 bits, unit stride on V, row stride logits_rs (any)
  const int* params;             // [0] fp32 bits of the temperature, [1] top_k (<= 0 or >= V: all)
  const float* u;                // (B,) uniforms in (0, 1), or null: Philox from seed / positions
  const long* seed;              // one 64-bit Philox key (with u == null)
  const int* positions;          // (B / R,): Philox counter word 0 and the history column, or null
  long* out_tokens;              // (B,) with stride out_s
  long* history;                 // (B, L) with row stride history_rs, or null (needs positions)
  float* u_out;                  // (B,) the u that was used, or null
  long logits_rs, out_s, history_rs;
  int B, V, L;
  // Rows per sequence (>= 1; 0 reads as 1): row r is token t = r % R of sequence r / R, and its
  // counter is (positions[r / R] + pos_off + t, r / R, 0, 0).  history needs R == 1.
  int R, pos_off;
};

}  // namespace orion
