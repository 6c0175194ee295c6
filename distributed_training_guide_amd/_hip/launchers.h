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

// moe_router.hip: top-k routing over bf16 logits [T, E], E in {8, 16, 32,
// 64, 128} and 1 <= k <= min(8, E).  topk_idx is int32 [T, k], topk_w and
// d_topk_w f32 [T, k]; `norm` selects the softmax over the k selected logits
// (otherwise the full softmax's values at the selection).  The backward
// writes every element of dlogits (bf16 [T, E]).  T == 0 launches nothing.
void moe_router_fwd_launch(const void* logits, int* topk_idx, float* topk_w,
                           int64_t T, int E, int k, int norm, hipStream_t s);
void moe_router_bwd_launch(const void* logits, const int* topk_idx,
                           const float* d_topk_w, void* dlogits, int64_t T,
                           int E, int k, int norm, hipStream_t s);

// moe_router_aux.hip: the same router, which also produces the
// load-balancing loss `aux` and the router z-loss `z` of the T >= 1 tokens
// (two f32 scalars) and counts int32 [E], the slots routed to each expert.
// topk_idx and topk_w are moe_router_fwd_launch's bits.  `partials` is
// moe_router_aux_grid(T, E) * (2E + 1) f32 of scratch that needs no
// initialisation.  The backward adds the two losses' terms to the routing
// term; g_aux and g_z are the upstream gradients as device scalars.
int moe_router_aux_grid(int64_t T, int E);
void moe_router_aux_fwd_launch(const void* logits, int* topk_idx,
                               float* topk_w, float* partials, int* counts,
                               float* aux, float* z, int64_t T, int E, int k,
                               int norm, hipStream_t s);
void moe_router_aux_bwd_launch(const void* logits, const int* topk_idx,
                               const float* d_topk_w, const int* counts,
                               const float* g_aux, const float* g_z,
                               void* dlogits, int64_t T, int E, int k,
                               int norm, hipStream_t s);

// moe_dispatch.hip.  moe_index_launch turns topk_idx (N = T*k slots, values
// in [0, E)) into dest int32 [N] (the slot's row in the expert-sorted
// layout) and offs int32 [E] (inclusive cumulative rows per expert); `hist`
// is moe_index_scratch(N, E) int32 of scratch that needs no initialisation.
// N == 0 is fine: offs comes out as zeros.
// moe_scatter_launch: bf16 rows of H % 8 == 0 elements, 16 B aligned.  With
// a null `w` it copies x[t] to xp[dest[t*k + j]] for every j and ignores
// `yp` and `dw` (null); with `w` (f32 [T, k]) it writes
// xp[dest[s]] = w[s] * x[t] and dw[s] = <x[t], yp[dest[s]]>.
// moe_combine_launch: y[t] = sum_j w[t, j] * yp[dest[t*k + j]]; a null `w`
// means weights of one.  dest must be a permutation of [0, N): the kernels
// index rows with it unchecked.
int64_t moe_index_scratch(int64_t N, int E);
void moe_index_launch(const int* topk_idx, int* dest, int* offs, int* hist,
                      int64_t N, int E, hipStream_t s);
void moe_scatter_launch(const void* x, const int* dest, const float* w,
                        const void* yp, void* xp, float* dw, int64_t T, int H,
                        int k, hipStream_t s);
void moe_combine_launch(const void* yp, const int* dest, const float* w,
                        void* y, int64_t T, int H, int k, hipStream_t s);

// moe_gemm.hip: the expert GEMMs over the expert-sorted rows.  a [N, K],
// weight [E, M, K], dy / y [N, M], all bf16, 16 B aligned, M and K multiples
// of 64, E <= 128; offs int32 [E] as moe_index_launch writes it, read on the
// device only (values outside [0, N] are clamped).
// moe_gemm_rows_launch: trans_b == 0 writes out [N, M] = rows . weight[e]^T
// from rows = a; trans_b != 0 writes out [N, K] = rows . weight[e] from
// rows = dy [N, M].  Rows that offs assigns to no expert are not written.
// moe_gemm_dw_launch: dw [E, M, K] = dy[rows of e]^T . a[rows of e], every
// element written once, zeros for an expert without rows.
void moe_gemm_rows_launch(const void* rows, const void* weight,
                          const int* offs, void* out, int64_t N, int E, int M,
                          int K, int trans_b, hipStream_t s);
void moe_gemm_dw_launch(const void* dy, const void* a, const int* offs,
                        void* dw, int64_t N, int E, int M, int K,
                        hipStream_t s);

// moe_gemm_gather.hip: the forward and dW of moe_gemm.hip with the token
// operand read through a row index instead of from the expert-sorted copy.
// x [T, K] bf16, 16 B aligned; row_src int32 [N], the token of every sorted
// row (values outside [0, T) are clamped); the rest as above.
// moe_row_src_launch: row_src[dest[t*k + j]] = t for dest int32 [T*k], a
// permutation of [0, T*k), k <= 8; every element written once.
// moe_gemm_rows_gather_launch: out [N, M] = x[row_src[r]] . weight[e]^T.
// moe_gemm_dw_gather_launch: dw [E, M, K] = dy[rows of e]^T .
// x[row_src[rows of e]], every element written once.
void moe_row_src_launch(const int* dest, int* row_src, int64_t T, int k,
                        hipStream_t s);
void moe_gemm_rows_gather_launch(const void* x, const int* row_src,
                                 const void* weight, const int* offs,
                                 void* out, int64_t N, int64_t T, int E, int M,
                                 int K, hipStream_t s);
void moe_gemm_dw_gather_launch(const void* dy, const void* x,
                               const int* row_src, const int* offs, void* dw,
                               int64_t N, int64_t T, int E, int M, int K,
                               hipStream_t s);

// moe_gemm_swiglu.hip: the gate_up forward and the down dA with the weighted
// SwiGLU in their epilogues.  gate_up [E, 2I, K], down [E, H, I], I, K and H
// multiples of 64; w_row f32 [N], the router weight of every sorted row; the
// rest as above.
// moe_row_w_launch: w_row[dest[t*k + j]] = topk_w[t, j], k <= 8.
// moe_gemm_gu_swiglu_launch: gu [N, 2I] = x[row_src[r]] . gate_up[e]^T (the
// bits of moe_gemm_rows_gather_launch) and hw [N, I] = w_row * silu(g) * u
// from the rounded gu.
// moe_gemm_da_swiglu_launch: from dyp [N, H] and the saved gu, dgu [N, 2I]
// (the SwiGLU backward of w_row * (dyp . down[e]), which is never written)
// and dw_topk f32 [N], dw_topk[s] = <dyp . down[e], silu(g) * u> of row
// dest[s].  dwp is N * moe_dw_parts(I) f32 of scratch that needs no
// initialisation.
void moe_row_w_launch(const int* dest, const float* topk_w, float* w_row,
                      int64_t T, int k, hipStream_t s);
void moe_gemm_gu_swiglu_launch(const void* x, const int* row_src,
                               const float* w_row, const void* gate_up,
                               const int* offs, void* gu, void* hw, int64_t N,
                               int64_t T, int E, int I, int K, hipStream_t s);
int moe_dw_parts(int I);
void moe_gemm_da_swiglu_launch(const void* dyp, const void* down,
                               const void* gu, const float* w_row,
                               const int* offs, const int* dest, void* dgu,
                               float* dwp, float* dw_topk, int64_t N, int E,
                               int H, int I, hipStream_t s);

// embedding.hip
void embed_fwd_launch(const void* table, const int64_t* ids, void* out,
                      int64_t nrows, int H, int64_t V, hipStream_t s);
void embed_bwd_launch(const void* dy, const int64_t* ids, float* acc,
                      void* dtable, int64_t nrows, int H, int64_t V,
                      hipStream_t s);

// embedding_bwd_sorted.hip: the same gradient without atomics, in an order
// fixed by ids (stable sort of the positions by id, then one wave per table
// row, long rows cut into pieces summed in parallel).  `scratch` is embed_bwd_sorted_scratch(N, V) int32 and `partials`
// embed_bwd_sorted_partials(N) rows of [H] f32 (null where that is 0);
// neither needs initialisation.  N = nrows < 2^31 - 1024 (N == 0 writes
// zeros), V <= 2^30; every row of dtable is written.
int64_t embed_bwd_sorted_scratch(int64_t N, int64_t V);
int64_t embed_bwd_sorted_partials(int64_t N);
void embed_bwd_sorted_launch(const void* dy, const int64_t* ids, int* scratch,
                             float* partials, void* dtable, int64_t N, int H,
                             int64_t V, hipStream_t s);

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

// fp8_delayed.hip: the one-pass forms for a scale known up front, same
// tensor requirements.  fp8_cast_amax_launch is fp8_cast_transpose_launch
// that also writes one sign-cleared bf16 bit pattern per 64x64 tile to
// `partials` (fp8_tiles(R, C) dwords, no initialisation needed).
// silu_mul_fp8_launch quantises h = silu(gate) * up of gu [R, 2I] (gate | up
// packed, R % 16 == 0 and I % 16 == 0) without writing h: q [R, I], qt
// [I, R], fp8_tiles(R, I) partials.  fp8_history_update_launch folds nparts
// >= 1 partials (16 B aligned) into this step's amax, writes it to
// history[slot] (f32 [L], L >= 1; slot < 0 fills every slot; a non-finite
// amax is replaced by the previous max(history)) and out[0] = 448 /
// max(max(history), 1e-12), out[1] = its reciprocal quotient.
int64_t fp8_tiles(int R, int C);
void fp8_cast_amax_launch(const void* x, const float* scale, void* q,
                          void* qt, void* partials, int R, int C,
                          hipStream_t s);
void silu_mul_fp8_launch(const void* gu, const float* scale, void* q, void* qt,
                         void* partials, int R, int I, hipStream_t s);
void fp8_history_update_launch(const void* partials, int nparts,
                               float* history, int L, int slot, float* out,
                               hipStream_t s);

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
