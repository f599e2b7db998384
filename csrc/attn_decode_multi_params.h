// Parameter block shared by csrc/attn_decode_multi.hip and csrc/bindings.cpp.
#pragma once

namespace orion {

// A few queries per row against a key/value cache with a causal tail, split over keys
// (attn_decode_multi_kernel).  Query t of row b attends keys [0, lim),
// lim = clamp(kv_lens[b] - Tq + 1 + t, 0, min(kv_lens[b], Tmax)).
struct DecodeMultiParams {
  const unsigned short* q;  // (B, Tq, Hq, D) bf16 bits, unit stride on D
  const unsigned short* k;  // (B, Tmax, Hkv, D)
  const unsigned short* v;
  unsigned short* o;        // (B, Tq, Hq, D) contiguous
  const int* kv_lens;       // (B,) on the device, the Tq tokens of this forward included
  float* ws_o;              // [B][Tq][Hq][splits][D] fp32 partial numerators (splits > 1)
  float* ws_ml;             // [B][Tq][Hq][splits][2] fp32 partial (max, sum), base-2 scores
  long q_sb, q_st, q_sh;
  long k_sb, k_st, k_sh;
  long v_sb, v_st, v_sh;
  int B, Tq, Hq, Hkv, Tmax;
  int splits;  // gridDim.x
  int chunk;   // keys per split, a whole number of key tiles
  float scale_log2;  // softmax scale * log2(e)
};

}  // namespace orion
