// Parameter blocks shared by csrc/attn_decode.hip and csrc/bindings.cpp.
#pragma once

namespace orion {

// Single-query attention over a key/value cache, split over keys (attn_decode_kernel).
struct DecodeParams {
  const unsigned short* q;  // (B, Hq, D) bf16 bits, unit stride on D
  const unsigned short* k;  // (B, Tmax, Hkv, D)
  const unsigned short* v;
  unsigned short* o;        // (B, Hq, D) contiguous
  const int* kv_lens;       // (B,) on the device; row b attends keys [0, min(kv_lens[b], Tmax))
  float* ws_o;              // [B][Hq][splits][D] fp32 partial numerators (splits > 1)
  float* ws_ml;             // [B][Hq][splits][2] fp32 partial (max, sum), base-2 scores
  long q_sb, q_sh;
  long k_sb, k_st, k_sh;
  long v_sb, v_st, v_sh;
  int B, Hq, Hkv, Tmax;
  int splits;  // gridDim.x
  int chunk;   // keys per split, a whole number of key tiles
  float scale_log2;  // softmax scale * log2(e)
};

// Append T new tokens per row to the cache at positions kv_lens[b] + t, rotating k (and q)
// on the way when tables are given (kv_append_kernel).
struct AppendParams {
  const unsigned short* k_new;  // (B, T, Hkv, D)
  const unsigned short* v_new;
  const unsigned short* q;      // (B, T, Hq, D) or null
  unsigned short* k_cache;      // (B, Tmax, Hkv, D)
  unsigned short* v_cache;
  unsigned short* q_out;        // (B, T, Hq, D) contiguous, or null
  const int* kv_lens;
  const float* cosv;  // [npos][D / 2] fp32 or null
  const float* sinv;
  long kn_sb, kn_st, kn_sh;
  long vn_sb, vn_st, vn_sh;
  long q_sb, q_st, q_sh;
  long kc_sb, kc_st, kc_sh;
  long vc_sb, vc_st, vc_sh;
  int B, T, Hq, Hkv, D, Tmax, npos;
};

}  // namespace orion
