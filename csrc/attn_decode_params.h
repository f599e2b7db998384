// Parameter blocks shared by csrc/attn_decode.hip and csrc/bindings.cpp.  A cache is bf16
// (B, Tmax, Hkv, D), or FP8: OCP e4m3fn bytes of that shape with one fp32 scale per (row, KV head,
// token) laid out (B, Hkv, Tmax), value = scale * byte.
#pragma once

namespace orion {

// Tq queries per row against a key/value cache, split over keys (attn_decode_kernel).  Query t of
// row b attends keys [0, lim), lim = clamp(kv_lens[b] - Tq + 1 + t, 0, min(kv_lens[b], Tmax)): with
// one query, every key below the length.
struct DecodeParams {
  const unsigned short* q;  // (B, Tq, Hq, D) bf16 bits, unit stride on D
  const void* k;            // (B, Tmax, Hkv, D) bf16 bits or e4m3 bytes, unit stride on D, rows aligned
  const void* v;            //   to a lane's load of 8 elements
  const float* k_scale;     // FP8: (B, Hkv, Tmax), unit stride on tokens; bf16: null
  const float* v_scale;
  unsigned short* o;        // (B, Tq, Hq, D) contiguous
  const int* kv_lens;       // (B,) on the device, the Tq tokens of this forward included
  float* ws_o;              // [B][Tq][Hq][splits][D] fp32 partial numerators (splits > 1)
  float* ws_ml;             // [B][Tq][Hq][splits][2] fp32 partial (max, sum), base-2 scores
  long q_sb, q_st, q_sh;    // single-query: Tq = 1, q_st is not read
  long k_sb, k_st, k_sh;
  long v_sb, v_st, v_sh;
  long ks_sb, ks_sh;
  long vs_sb, vs_sh;
  int B, Tq, Hq, Hkv, Tmax;
  int splits;  // gridDim.x
  int chunk;   // keys per split, a whole number of key tiles
  float scale_log2;  // softmax scale * log2(e)
};

// Append T new bf16 tokens per row to the cache at positions kv_lens[b] + t, rotating k (and q) in
// fp32 on the way when tables are given (kv_append_kernel); into an FP8 cache each head row is
// quantised by its own amax (kv_append_fp8_kernel).
struct AppendParams {
  const unsigned short* k_new;  // (B, T, Hkv, D)
  const unsigned short* v_new;
  const unsigned short* q;      // (B, T, Hq, D) or null
  void* k_cache;                // (B, Tmax, Hkv, D) bf16 bits or e4m3 bytes
  void* v_cache;
  float* k_scale;               // FP8: (B, Hkv, Tmax); bf16: null
  float* v_scale;
  unsigned short* q_out;        // (B, T, Hq, D) contiguous, or null
  const int* kv_lens;
  const float* cosv;  // [npos][D / 2] fp32 or null
  const float* sinv;
  long kn_sb, kn_st, kn_sh;
  long vn_sb, vn_st, vn_sh;
  long q_sb, q_st, q_sh;
  long kc_sb, kc_st, kc_sh;
  long vc_sb, vc_st, vc_sh;
  long ks_sb, ks_sh;
  long vs_sb, vs_sh;
  int B, T, Hq, Hkv, D, Tmax, npos;
};

}  // namespace orion
