// C-linkage entry points of the HIP extension, declared once.
//
// bindings.cpp calls these; every .hip file that defines one includes this
// header, so a definition that drifts from its declaration is a compile
// error (conflicting types for a C-linkage function) rather than a call
// that links and passes garbage.  bf16 tensors travel as void*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// colsum_launch folds its input in two stages through COLSUM_RY rows of
// f32 scratch.  Every `partial` buffer below is
// [nblocks + COLSUM_RY, H] f32: the kernels write rows [0, nblocks), the
// tail is that scratch.
#define COLSUM_RY 16

extern "C" {
// colsum.hip: out[H] (bf16) = column sums of partial[0:nblocks, H]
void colsum_launch(float* partial, void* out, int nblocks, int H,
                   hipStream_t s);

// norm.hip.  One forward and one backward entry point serve RMSNorm and
// LayerNorm: a null `mu` (and `b`) selects RMSNorm, otherwise LayerNorm.  In
// the backward a non-null `dres` selects RMSNorm's fused residual form,
// dx += dres (H % 8 == 0 and H <= 16384 only; LayerNorm has none, so `dres`
// is null whenever `mu` is not).  `db_partial` / `db` are LayerNorm's and
// null for RMSNorm.  With nblocks == 0 (no rows) the backward launches no
// norm kernel and dw (db) come out as zeros.
void norm_fwd_launch(const void* x, const void* w, const void* b, void* y,
                     float* mu, float* rstd, int64_t nrows, int H, float eps,
                     hipStream_t s);
void add_rmsnorm_fwd_launch(const void* res, const void* delta, const void* w,
                            void* res_out, void* y, void* rstd, int64_t nrows,
                            int H, float eps, hipStream_t s);
void norm_bwd_launch(const void* dy, const void* dres, const void* x,
                     const void* w, const float* mu, const float* rstd,
                     void* dx, float* dw_partial, float* db_partial, void* dw,
                     void* db, int nblocks, int64_t nrows, int H,
                     hipStream_t s);

// gelu.hip
void gelu_fwd_launch(const void* x, void* y, int64_t n, hipStream_t s);
void gelu_bwd_launch(const void* dy, const void* x, void* dx, int64_t n,
                     hipStream_t s);

// rope.hip, qkv_rope.hip
void rope_launch(const void* x, void* y, const float* cs, const float* sn,
                 const int* positions, int64_t total_rows, int S, int H, int D,
                 int backward, hipStream_t stream);
void qkv_rope_fwd_launch(const void* qkv, void* q, void* k, void* v,
                         const float* cs, const float* sn,
                         const int* positions, int64_t BS, int S, int Hq,
                         int Hkv, int D, hipStream_t stream);
void qkv_rope_bwd_launch(const void* dq, const void* dk, const void* dv,
                         void* dqkv, const float* cs, const float* sn,
                         const int* positions, int64_t BS, int S, int Hq,
                         int Hkv, int D, hipStream_t stream);

// qkv_norm_rope.hip: the qkv split with a per-head RMSNorm (weights wq / wk,
// bf16 [D]) on every q and k row before the rotation; D is 64 or 128 and
// qkv is [B,S,W].  The backward reads the saved qkv, writes
// qkv_norm_rope_bwd_blocks(B, S) rows of `dw_partial` ([blocks + COLSUM_RY,
// 2*D] f32, no initialisation needed) and finishes them with colsum_launch
// into `dw` (bf16 [2*D]: dwq | dwk).  With B or S zero nothing is launched.
int qkv_norm_rope_bwd_blocks(int64_t B, int S);
void qkv_norm_rope_fwd_launch(const void* qkv, const void* wq, const void* wk,
                              void* q, void* k, void* v, const float* cs,
                              const float* sn, const int* positions,
                              int64_t B, int S, int Hq, int Hkv, int D,
                              float eps, hipStream_t stream);
void qkv_norm_rope_bwd_launch(const void* dq, const void* dk, const void* dv,
                              const void* qkv, const void* wq, const void* wk,
                              void* dqkv, float* dw_partial, void* dw,
                              const float* cs, const float* sn,
                              const int* positions, int64_t B, int S, int Hq,
                              int Hkv, int D, float eps, hipStream_t stream);

// silu_mul.hip
void silu_mul_fwd_launch(const void* gu, void* y, int64_t nrows, int I,
                         hipStream_t s);
void silu_mul_bwd_launch(const void* dy, const void* gu, void* dgu,
                         int64_t nrows, int I, hipStream_t s);

// embedding.hip
void embed_fwd_launch(const void* table, const int64_t* ids, void* out,
                      int64_t nrows, int H, int64_t V, hipStream_t s);
void embed_bwd_launch(const void* dy, const int64_t* ids, float* acc,
                      void* dtable, int64_t nrows, int H, int64_t V,
                      hipStream_t s);

// cross_entropy.hip
void ce_fwd_launch(const void* logits, const int64_t* labels, float* loss,
                   float* lse, int64_t nrows, int S_logits, int S_out, int V,
                   int64_t ignore_index, hipStream_t st);
void ce_fwd_sharded_launch(const void* logits, const int64_t* labels,
                           float* maxout, float* sumout, float* gathered,
                           int64_t nrows, int S_logits, int S_out, int V,
                           int64_t vocab_start, int64_t ignore_index,
                           hipStream_t st);
void ce_bwd_launch(const void* logits, const int64_t* labels, const float* lse,
                   void* dlogits, float scale, const float* scale_ptr,
                   int64_t nrows, int S_logits, int S_out, int V,
                   int64_t vocab_start, int64_t ignore_index, int sharded,
                   hipStream_t st);

// adamw.hip, grad_norm.hip
void adamw_launch(const void* descs, int nchunks, float lr, float beta1,
                  float beta2, float eps, float wd, float inv_bc1,
                  float inv_bc2, hipStream_t s);
void adamw_launch_clipped(const void* descs, int nchunks, float lr,
                          float beta1, float beta2, float eps, float wd,
                          float inv_bc1, float inv_bc2, const float* sq_total,
                          float max_norm, hipStream_t s);
// Master-weight form: lo_tab is an [nchunks] table of device pointers to the
// int16 companions of the bf16 chunks (0 for an fp32 chunk, which has none).
// A null sq_total selects the unclipped instantiation.
void adamw_master_launch(const void* descs, const int64_t* lo_tab,
                         int nchunks, float lr, float beta1, float beta2,
                         float eps, float wd, float inv_bc1, float inv_bc2,
                         const float* sq_total, float max_norm,
                         hipStream_t s);
void grad_sqsum_launch(const void* descs, int nchunks, float* partials,
                       float* out, int slot, hipStream_t s);
void grad_scale_launch(const void* descs, int nchunks, const float* sq_total,
                       float max_norm, hipStream_t s);

// fp8_quant.hip: tensor-wise e4m3 quantisation of a contiguous, 16 B aligned
// bf16 [R, C] tensor, R % 16 == 0 and C % 16 == 0.  fp8_amax_scale_launch
// writes scales[0] = 448 / max(amax, 1e-12) and scales[1] = its reciprocal
// quotient; `partials` holds fp8_amax_blocks(numel) dwords and needs no
// initialisation.  fp8_cast_transpose_launch writes the row-major e4m3
// [R, C] to `q` and the transposed [C, R] to `qt`; a null pointer drops that
// output (both null launches nothing).
int fp8_amax_blocks(int64_t numel);
void fp8_amax_scale_launch(const void* x, int64_t numel, void* partials,
                           float* scales, hipStream_t s);
void fp8_cast_transpose_launch(const void* x, const float* scale, void* q,
                               void* qt, int R, int C, hipStream_t s);

// attention_fwd.hip, attention_bwd.hip.  doc_start / doc_end are the [B,S]
// int32 tables of the document-masked mode for packed rows (first token /
// exclusive end of each token's document); null selects the plain causal
// kernels.  The backward takes both or neither.
void attn_fwd_launch(const void* q, const void* k, const void* v, void* o,
                     float* lse, const int* doc_start, int B, int S, int Hq,
                     int Hkv, int D, float scale, hipStream_t stream);
void attn_bwd_launch(const void* dout, const void* q, const void* k,
                     const void* v, const void* o, const float* lse,
                     float* delta, void* dq, void* dk, void* dv,
                     const int* doc_start, const int* doc_end, int B, int S,
                     int Hq, int Hkv, int D, float scale, hipStream_t stream);
}
