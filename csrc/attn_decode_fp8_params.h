// Parameter blocks shared by csrc/attn_decode_fp8.hip and csrc/bindings.cpp: the FP8 (OCP e4m3fn)
// key/value cache, bytes (B, Tmax, Hkv, D) with one fp32 scale per (row, KV head, token) laid out
// (B, Hkv, Tmax): value = scale * byte.
#pragma once

namespace orion {

// Single-query attention over an FP8 cache, split over keys (attn_decode_fp8_kernel).
struct DecodeFp8Params {
  const unsigned short* q;   // (B, Hq, D) bf16 bits, unit stride on D
  const unsigned char* k;    // (B, Tmax, Hkv, D) e4m3 bytes, unit stride on D, 8-byte aligned rows
  const unsigned char* v;
  const float* k_scale;      // (B, Hkv, Tmax), unit stride on tokens
  const float* v_scale;
  unsigned short* o;         // (B, Hq, D) contiguous
  const int* kv_lens;        // (B,) on the device; row b attends keys [0, min(kv_lens[b], Tmax))
  float* ws_o;               // [B][Hq][splits][D] fp32 partial numerators (splits > 1)
  float* ws_ml;              // [B][Hq][splits][2] fp32 partial (max, sum), base-2 scores
  long q_sb, q_sh;
  long k_sb, k_st, k_sh;
  long v_sb, v_st, v_sh;
  long ks_sb, ks_sh;
  long vs_sb, vs_sh;
  int B, Hq, Hkv, Tmax;
  int splits;  // gridDim.x
  int chunk;   // keys per split, a whole number of key tiles
  float scale_log2;  // softmax scale * log2(e)
};

// Append T new bf16 tokens per row to the FP8 cache at positions kv_lens[b] + t, k rotated in fp32
// when tables are given, each head row quantised by its own amax (kv_append_fp8_kernel).
struct AppendFp8Params {
  const unsigned short* k_new;  // (B, T, Hkv, D) bf16
  const unsigned short* v_new;
  const unsigned short* q;      // (B, T, Hq, D) or null
  unsigned char* k_cache;       // (B, Tmax, Hkv, D) e4m3 bytes
  unsigned char* v_cache;
  float* k_scale;               // (B, Hkv, Tmax)
  float* v_scale;
  unsigned short* q_out;        // (B, T, Hq, D) bf16 contiguous, or null
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
