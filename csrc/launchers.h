// The one declaration of every host entry point of csrc/*.hip and csrc/blaslt.cpp that crosses a file
// boundary.  Each defining file includes it, as do the callers (csrc/bindings.cpp, other kernel files,
// tests/native/host_logic.cpp); default arguments live here only.  No torch, no device code.
// A launcher returns 0, a HIP error code (> 0), or a negative code: as a rule -1 shape, -2 alignment or
// 32-bit offset overflow, -3 missing operand, -4 slabs / workspace; any other negative is a failure too
// (-5 a kernel attribute or an oversized plan; lmhead_fold -2 a failed memset).  Callers test for != 0.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_decode_params.h"
#include "attn_plan.h"
#include "linear_decode_fp8_params.h"
#include "linear_decode_mxfp4_params.h"
#include "linear_decode_params.h"
#include "sample_params.h"

// layernorm.hip: LayerNorm, the column-sum fold and its scratch sizes (in floats)
int orion_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, int rows,
                        int C, float eps, const void* res, void* sum_out, const void* rbias, hipStream_t st,
                        const int64_t* idx = nullptr, int T = 0, long V = 0, int* err = nullptr);  // -1: C
int orion_layernorm_bwd_blocks(int rows);
long orion_layernorm_bwd_scratch(int rows, int C);  // of `part` below
int orion_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd,
                        void* dx, void* dw, void* db, float* part, int rows, int C, const void* dres,
                        void* drbias, int grad_f32, hipStream_t st);  // -1: C
long orion_colsum_mid_scratch(int C, int outputs);  // what a fold of `outputs` sums of C columns may write
int orion_colsum_scratch(int rows, int C);          // partials of `rows` rows + mid: `part` of a bf16 colsum
int orion_colsum_bf16(const void* m, void* out, float* part, int rows, int C, int out_f32, hipStream_t st);
// out[C] = column sums of part[P][C]; mid: orion_colsum_mid_scratch(C, 1)
int orion_colsum_partials2(const float* part, float* mid, void* out, int P, int C, int f32, hipStream_t st);

// embedding.hip
int orion_embed_scatter_add(const void* dx, const int64_t* idx, float* out, long rows, int C, long V, int* err,
                            hipStream_t st);
int orion_batch_sum(const void* x, void* out, int B, long n, int out_f32, hipStream_t st);

// activations.hip (-1: a length that is no multiple of the vector width)
int orion_bias_gelu_fwd(const void* x, const void* b, void* y, long n, int C, hipStream_t st);
int orion_bias_gelu_bwd(const void* dy, const void* x, const void* b, void* dx, float* part, int rows, int C,
                        hipStream_t st);
int orion_swiglu_fwd(const void* gu, void* y, long rows, int F, hipStream_t st);
int orion_swiglu_bwd(const void* dy, const void* gu, void* dgu, long rows, int F, hipStream_t st);
int orion_scale_bf16(void* x, const float* scale, long n, hipStream_t st);
int orion_slab_sum(const float* slabs, int S, long n, void* out, const float* scale, int accumulate, int out_f32,
                   hipStream_t st);

// wgrad.hip: dW = A^T B over M tokens and its split-K planning
int orion_wgrad_splits(int M, int N1, int N2);
int orion_wgrad_effective_splits(int M, int S);
int orion_wgrad_tail_rows(int M, int N1, int N2, int* S2);
// -1 shape (M % BK, N % 8, ld % 8), -2 alignment, -3 S is no effective split count, -4 S > 1 without slabs
int orion_wgrad(const void* A, long lda, const void* B, long ldb, int M, int N1, int N2, int S, float* slabs,
                void* out, const float* scale, int accumulate, int out_f32, int bt, hipStream_t st);

// xent.hip, adamw.hip
int orion_xent_fwd_bwd(void* logits, const int64_t* targets, float* losses, float* inv_n, float* loss_out, long N,
                       int V, long ignore, int* err, hipStream_t st);
int orion_sumsq_partials();  // floats of `partial` below
int orion_grad_sumsq(const void* g, long n, int g_f32, float* partial, float* out, hipStream_t st);
int orion_adamw_flat(void* p16, float* master, float* m, float* v, const void* g, int g_f32, const uint8_t* decay,
                     const float* hyper, const float* sumsq, long n, hipStream_t st);

// rmsnorm_rope.hip (-1: C % 8 or D % 16, -2: C beyond 8 vector passes, -3: a null rope operand)
int orion_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int rows, int C, float eps,
                      const void* res, void* sum_out, hipStream_t st);
int orion_rmsnorm_bwd_blocks(int rows);
long orion_rmsnorm_bwd_scratch(int rows, int C);  // of `part` below
int orion_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, void* dw,
                      float* part, int rows, int C, const void* dres, int dw_f32, hipStream_t st);
int orion_rope(const void* x, long xsb, long xst, long xsh, void* y, long ysb, long yst, long ysh,
               const float* cosv, const float* sinv, int B, int T, int H, int D, int pos0, float sign,
               hipStream_t st);

// attn_fwd.hip, attn_bwd_split.hip, attention.hip (64-bit addressing; fused backward).  What runs is
// decided by csrc/attn_plan.h; -1: a head dim, or a kernel id, that the file has no kernel for
int orion_attn_fwd(const orion::AttnParams& p, int D, bool causal, hipStream_t st);  // plans, then launches
int orion_attn_fwd64(const orion::AttnLaunch& l, const orion::AttnParams& p, int D, bool causal, hipStream_t st);
// the steps of an orion::attn_bwd_plan of form ATTN_SPLIT / ATTN_FUSED; delta: [B][Hq][T] fp32 scratch
int orion_attn_bwd_split(const orion::AttnBwdPlan& plan, const orion::AttnParams& p, int D, bool causal,
                         float* delta, hipStream_t st);
int orion_attn_bwd(const orion::AttnBwdPlan& plan, const orion::AttnParams& p, int D, bool causal, float* delta,
                   hipStream_t st);
int orion_attn_dq_convert(const float* acc, void* dq, long sb, long st_, long sh, int B, int Hq, int T, int D,
                          hipStream_t st);

// gemm.hip, in front of gemm16.hip: -1 shape / leading dims, -2 alignment, -3 an operand the epilogue needs
int orion_gemm(const void* X, long ldx, const void* W, long ldw, int M, int N, int K, int wkm, int epi, void* out,
               long ldo, const void* bias, void* out2, long ldo2, const void* pre, long ldp, hipStream_t st,
               void* db = nullptr, int db_f32 = 0, float* part = nullptr);
int orion_gemm_colsum_scratch(int M, int N);  // floats of orion_gemm's `part`
int orion_gemm_lm(const void* X, long ldx, const void* W, long ldw, int M, int N, int K, int epi, void* out,
                  long ldo, float* rowpart, const int64_t* tgt, float* tlog, const float* cref, const float* rs,
                  hipStream_t st);
int orion_gemm_rope(const void* X, long ldx, const void* W, long ldw, int M, int N, int K, void* out, long ldo,
                    const float* cosv, const float* sinv, int T, int pos0, int rcols, int D, hipStream_t st);
int orion_gemm_swiglu(const void* X, long ldx, const void* W, long ldw, int M, int F, int K, void* gu, long ldg,
                      void* h, long ldh, hipStream_t st);
int orion_gemm_set_diag(int flags);  // returns the previous flags; flags < 0 only queries

// blaslt.cpp: D = X W^T (+ bias) (+ R) through hipBLASLt (-1 shape, -2 device, <= -10 library)
int orion_blaslt_linear_res(const void* X, long ldx, const void* W, long ldw, const void* bias, const void* R,
                            long ldr, void* D, long ldd, int M, int N, int K, hipStream_t st);

// lmhead.hip
int orion_lmhead_fold(const float* part, int npart, const float* tlog, const int64_t* tgt, long ignore,
                      float* cref, void* E, long lde, int V, long N, const void* X, long ldx, const void* W,
                      long ldw, int Cdim, float* invz, float* lse, float* loss_rows, int* counts, int* fix_list,
                      float* loss_out, float* inv_n, int* err, hipStream_t st);
int orion_lmhead_bwd_prep(const void* X, long ldx, int Cdim, long N, const int64_t* tgt, long ignore, int V,
                          const float* invz, const float* inv_n, const float* g, float* srow, void* Xs,
                          int transposed, hipStream_t st);

// attn_decode.hip, linear_decode.hip, linear_decode_fp8.hip, linear_decode_mxfp4.hip, sample.hip,
// spec_decode.hip: generation
// (negative: a field of p failed its check)
int orion_attn_decode_split_plan(int tile, int B, int Hkv, int Tmax, int splits, int* chunk);  // key tiles of `tile`
int orion_attn_decode_plan(int B, int Hkv, int Tmax, int D, int splits, int* chunk);  // of all three ops below
// one query per row (Tq = 1) on a bf16 cache, on an FP8 cache (-6: no scales), and Tq <= 16 queries per row
// with a causal tail on a bf16 cache (-2 also: a chunk that is no whole number of key tiles)
int orion_attn_decode(const orion::DecodeParams& p, int D, hipStream_t st);
int orion_attn_decode_fp8(const orion::DecodeParams& p, int D, hipStream_t st);
int orion_attn_decode_multi(const orion::DecodeParams& p, int D, hipStream_t st);
int orion_attn_decode_combine(const float* ws_o, const float* ws_ml, void* o, int splits, int D, long heads,
                              hipStream_t st);
int orion_kv_append(const orion::AppendParams& p, hipStream_t st);
int orion_kv_append_fp8(const orion::AppendParams& p, hipStream_t st);  // -6: no scales
int orion_linear_decode(const orion::LinearDecodeParams& p, hipStream_t st);
int orion_linear_decode_fp8(const orion::LinearDecodeFp8Params& p, hipStream_t st);  // -1 also K % 16
int orion_linear_decode_mxfp4(const orion::LinearDecodeMxfp4Params& p, hipStream_t st);  // -1 also K % 32
int orion_sample_tokens(const orion::SampleParams& p, hipStream_t st);
// spec_decode.hip: out (B, k1) = the current token and k1 - 1 n-gram drafts; the accept rule of a verify step
int orion_spec_draft(const long* history, long hist_rs, const int* cur, long* out, long out_rs, int B, int L,
                     int k1, int ngram, hipStream_t st);
int orion_spec_accept(const long* tokens, long tok_rs, const long* target, long tgt_rs, const int* start,
                      int* lens, const int* stop, long* history, long hist_rs, int B, int k, int L,
                      hipStream_t st);
