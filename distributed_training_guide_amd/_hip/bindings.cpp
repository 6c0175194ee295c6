// PyTorch bindings for the gfx950 HIP kernels (compiled with hipcc,
// linked against libtorch; no hipify, no CUDA compatibility layer —
// c10::hip is the native ROCm stream API).
#include <torch/extension.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "launchers.h"

namespace {

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_BF16_CONTIG(t)                                          \
  TORCH_CHECK((t).is_cuda(), #t " must be on the GPU");               \
  TORCH_CHECK((t).dtype() == torch::kBFloat16, #t " must be bf16");   \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// cos / sin rope tables: f32 [max_pos, D/2], on x's device, equal shapes
#define CHECK_ROPE_TABLES(cos, sin, x, D)                                  \
  TORCH_CHECK((D) % 2 == 0, "rope head dim must be even");                 \
  TORCH_CHECK((cos).is_cuda() && (cos).device() == (x).device() &&         \
                  (sin).is_cuda() && (sin).device() == (x).device(),       \
              "rope tables must be on " #x "'s device");                   \
  TORCH_CHECK((cos).dtype() == torch::kFloat &&                            \
                  (sin).dtype() == torch::kFloat,                          \
              "rope tables must be f32");                                  \
  TORCH_CHECK((cos).is_contiguous() && (sin).is_contiguous(),              \
              "rope tables must be contiguous");                           \
  TORCH_CHECK((cos).dim() == 2 && (cos).size(1) == (D) / 2 &&              \
                  (sin).sizes() == (cos).sizes(),                          \
              "rope tables must both be [max_pos, D/2]")

// optional int32 [S] absolute positions on x's device; without them the
// table itself must cover the sequence
inline const int* rope_positions(const c10::optional<torch::Tensor>& positions,
                                 const torch::Tensor& cos,
                                 const torch::Tensor& x, int64_t S) {
  if (!positions.has_value()) {
    TORCH_CHECK(cos.size(0) >= S, "rope table shorter than sequence");
    return nullptr;
  }
  TORCH_CHECK(positions->is_cuda() && positions->device() == x.device(),
              "positions must be on the input's device");
  TORCH_CHECK(positions->dtype() == torch::kInt && positions->is_contiguous(),
              "positions must be contiguous int32");
  TORCH_CHECK(positions->numel() == S, "positions must be [S]");
  return positions->data_ptr<int>();
}

// what every cross-entropy entry point requires of logits / labels / S_out
#define CHECK_CE_INPUTS(logits, labels, S_out)                             \
  CHECK_BF16_CONTIG(logits);                                               \
  TORCH_CHECK((logits).dim() == 3, "logits must be [B,S,V]");              \
  TORCH_CHECK((labels).is_cuda() && (labels).device() == (logits).device(),\
              "labels must be on the logits' device");                     \
  TORCH_CHECK((labels).dtype() == torch::kLong && (labels).is_contiguous(),\
              "labels must be contiguous int64");                          \
  TORCH_CHECK((labels).dim() == 2 &&                                       \
                  (labels).size(0) == (logits).size(0) &&                  \
                  (labels).size(1) == (logits).size(1),                    \
              "labels must be [B,S]");                                     \
  TORCH_CHECK((S_out) > 0 && (S_out) <= (logits).size(1),                  \
              "S_out must be in (0, S]");                                  \
  TORCH_CHECK((logits).size(2) % 8 == 0,                                   \
              "vocab must be padded to a multiple of 8")

// [nblocks, H] f32 per-block partials of a norm backward, plus the
// COLSUM_RY tail rows colsum_launch folds them through
inline torch::Tensor alloc_partials(int nblocks, int H,
                                    const torch::Tensor& like) {
  return torch::empty({(int64_t)nblocks + COLSUM_RY, (int64_t)H},
                      like.options().dtype(torch::kFloat));
}

// ---------------- norms (norm.hip) ----------------
struct NormDims {
  int64_t nrows;
  int H;
};

// What every norm entry point requires before it launches.  x is the
// [..., H] input; `wb` the weight (and LayerNorm's bias), each exactly [H];
// `like_x` the tensors that travel with x (dy, dres_out, delta): x's sizes;
// `stats` the saved rstd (and mu): f32, one value per row.  All on x's device.
NormDims norm_check(const torch::Tensor& x,
                    std::initializer_list<torch::Tensor> wb,
                    std::initializer_list<torch::Tensor> like_x = {},
                    std::initializer_list<torch::Tensor> stats = {}) {
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0,
              "norm input must be [..., H] with H > 0");
  const int H = (int)x.size(-1);
  const int64_t nrows = x.numel() / H;
  for (const auto& weight_or_bias : wb) {
    CHECK_BF16_CONTIG(weight_or_bias);
    TORCH_CHECK(weight_or_bias.dim() == 1 && weight_or_bias.size(0) == H &&
                    weight_or_bias.device() == x.device(),
                "norm weight / bias must be [H] on the input's device");
  }
  for (const auto& dy_or_residual : like_x) {
    CHECK_BF16_CONTIG(dy_or_residual);
    TORCH_CHECK(dy_or_residual.sizes() == x.sizes() &&
                    dy_or_residual.device() == x.device(),
                "norm: dy / dres_out / delta must have the input's sizes "
                "and device");
  }
  for (const auto& t : stats) {
    TORCH_CHECK(t.is_cuda() && t.device() == x.device(),
                "norm: rstd / mu must be on the input's device");
    TORCH_CHECK(t.dtype() == torch::kFloat && t.is_contiguous(),
                "norm: rstd / mu must be contiguous f32");
    TORCH_CHECK(t.numel() == nrows,
                "norm: rstd / mu must hold one value per row");
  }
  return {nrows, H};
}

// the fused residual kernels are vector-only and stage a row in LDS
inline void add_rmsnorm_check_H(int H) {
  TORCH_CHECK(H % 8 == 0 && H <= 16384, "add_rmsnorm: unsupported H");
}

inline int norm_bwd_blocks(int64_t nrows) {
  return (int)std::min<int64_t>(nrows, 2048);
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps) {
  const NormDims d = norm_check(x, {w});
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({d.nrows}, x.options().dtype(torch::kFloat));
  norm_fwd_launch(x.data_ptr(), w.data_ptr(), nullptr, y.data_ptr(), nullptr,
                  rstd.data_ptr<float>(), d.nrows, d.H, (float)eps,
                  cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {y, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor rstd) {
  const NormDims d = norm_check(x, {w}, {dy}, {rstd});
  const int nblocks = norm_bwd_blocks(d.nrows);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty_like(w);
  auto dw_partial = alloc_partials(nblocks, d.H, x);
  norm_bwd_launch(dy.data_ptr(), nullptr, x.data_ptr(), w.data_ptr(), nullptr,
                  rstd.data_ptr<float>(), dx.data_ptr(),
                  dw_partial.data_ptr<float>(), nullptr, dw.data_ptr(),
                  nullptr, nblocks, d.nrows, d.H, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dw};
}

std::vector<torch::Tensor> add_rmsnorm_fwd(torch::Tensor res,
                                           torch::Tensor delta,
                                           torch::Tensor w, double eps) {
  const NormDims d = norm_check(res, {w}, {delta});
  add_rmsnorm_check_H(d.H);
  auto res_out = torch::empty_like(res);
  auto y = torch::empty_like(res);
  auto rstd = torch::empty({d.nrows}, res.options().dtype(torch::kFloat));
  add_rmsnorm_fwd_launch(res.data_ptr(), delta.data_ptr(), w.data_ptr(),
                         res_out.data_ptr(), y.data_ptr(), rstd.data_ptr(),
                         d.nrows, d.H, (float)eps, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {y, res_out, rstd};
}

std::vector<torch::Tensor> add_rmsnorm_bwd(torch::Tensor dy,
                                           torch::Tensor dres_out,
                                           torch::Tensor res_out,
                                           torch::Tensor w,
                                           torch::Tensor rstd) {
  const NormDims d = norm_check(res_out, {w}, {dy, dres_out}, {rstd});
  add_rmsnorm_check_H(d.H);
  const int nblocks = norm_bwd_blocks(d.nrows);
  auto dx = torch::empty_like(res_out);
  auto dw = torch::empty_like(w);
  auto dw_partial = alloc_partials(nblocks, d.H, res_out);
  norm_bwd_launch(dy.data_ptr(), dres_out.data_ptr(), res_out.data_ptr(),
                  w.data_ptr(), nullptr, rstd.data_ptr<float>(),
                  dx.data_ptr(), dw_partial.data_ptr<float>(), nullptr,
                  dw.data_ptr(), nullptr, nblocks, d.nrows, d.H,
                  cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dw};
}

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps) {
  const NormDims d = norm_check(x, {w, b});
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat);
  auto mu = torch::empty({d.nrows}, opts);
  auto rstd = torch::empty({d.nrows}, opts);
  norm_fwd_launch(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(),
                  mu.data_ptr<float>(), rstd.data_ptr<float>(), d.nrows, d.H,
                  (float)eps, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {y, mu, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mu,
                                         torch::Tensor rstd) {
  const NormDims d = norm_check(x, {w}, {dy}, {mu, rstd});
  const int nblocks = norm_bwd_blocks(d.nrows);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty_like(w);
  auto db = torch::empty_like(w);
  auto dw_partial = alloc_partials(nblocks, d.H, x);
  auto db_partial = alloc_partials(nblocks, d.H, x);
  norm_bwd_launch(dy.data_ptr(), nullptr, x.data_ptr(), w.data_ptr(),
                  mu.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr(),
                  dw_partial.data_ptr<float>(), db_partial.data_ptr<float>(),
                  dw.data_ptr(), db.data_ptr(), nblocks, d.nrows, d.H,
                  cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dx, dw, db};
}

// ---------------- rope ----------------
torch::Tensor rope(torch::Tensor x, torch::Tensor cos, torch::Tensor sin,
                   c10::optional<torch::Tensor> positions, bool backward) {
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(x.dim() == 4, "rope expects [B,S,H,D]");
  const int S = (int)x.size(1), H = (int)x.size(2), D = (int)x.size(3);
  CHECK_ROPE_TABLES(cos, sin, x, D);
  const int* pos_ptr = rope_positions(positions, cos, x, S);
  auto y = torch::empty_like(x);
  rope_launch(x.data_ptr(), y.data_ptr(), cos.data_ptr<float>(),
              sin.data_ptr<float>(), pos_ptr, x.numel() / D, S, H, D,
              backward ? 1 : 0, cur_stream());
  return y;
}

// ---------------- fused qkv split + rope ----------------
std::vector<torch::Tensor> qkv_rope_fwd(torch::Tensor qkv, torch::Tensor cos,
                                        torch::Tensor sin,
                                        c10::optional<torch::Tensor> positions,
                                        int64_t Hq, int64_t Hkv, int64_t D) {
  CHECK_BF16_CONTIG(qkv);
  TORCH_CHECK(qkv.dim() == 3, "qkv_rope expects [B,S,W]");
  const int64_t B = qkv.size(0), S = qkv.size(1);
  TORCH_CHECK(qkv.size(2) == (Hq + 2 * Hkv) * D, "packed width mismatch");
  TORCH_CHECK(D % 16 == 0,
              "qkv_rope requires head_dim % 16 == 0 (8-pair vectorized "
              "kernel); use the unfused rope path otherwise");
  CHECK_ROPE_TABLES(cos, sin, qkv, D);
  const int* pos_ptr = rope_positions(positions, cos, qkv, S);
  auto q = torch::empty({B, S, Hq, D}, qkv.options());
  auto k = torch::empty({B, S, Hkv, D}, qkv.options());
  auto v = torch::empty({B, S, Hkv, D}, qkv.options());
  qkv_rope_fwd_launch(qkv.data_ptr(), q.data_ptr(), k.data_ptr(),
                      v.data_ptr(), cos.data_ptr<float>(),
                      sin.data_ptr<float>(), pos_ptr, B * S, (int)S, (int)Hq,
                      (int)Hkv, (int)D, cur_stream());
  return {q, k, v};
}

torch::Tensor qkv_rope_bwd(torch::Tensor dq, torch::Tensor dk,
                           torch::Tensor dv, torch::Tensor cos,
                           torch::Tensor sin,
                           c10::optional<torch::Tensor> positions) {
  CHECK_BF16_CONTIG(dq);
  CHECK_BF16_CONTIG(dk);
  CHECK_BF16_CONTIG(dv);
  TORCH_CHECK(dq.dim() == 4, "dq must be [B,S,Hq,D]");
  TORCH_CHECK(dk.dim() == 4 && dk.size(0) == dq.size(0) &&
                  dk.size(1) == dq.size(1) && dk.size(3) == dq.size(3),
              "dk must be [B,S,Hkv,D]");
  TORCH_CHECK(dv.sizes() == dk.sizes(), "dv must be [B,S,Hkv,D]");
  TORCH_CHECK(dk.device() == dq.device() && dv.device() == dq.device(),
              "dk and dv must be on dq's device");
  const int64_t B = dq.size(0), S = dq.size(1);
  const int64_t Hq = dq.size(2), Hkv = dk.size(2), D = dq.size(3);
  TORCH_CHECK(D % 16 == 0, "qkv_rope requires head_dim % 16 == 0");
  CHECK_ROPE_TABLES(cos, sin, dq, D);
  const int* pos_ptr = rope_positions(positions, cos, dq, S);
  auto dqkv = torch::empty({B, S, (Hq + 2 * Hkv) * D}, dq.options());
  qkv_rope_bwd_launch(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                      dqkv.data_ptr(), cos.data_ptr<float>(),
                      sin.data_ptr<float>(), pos_ptr, B * S, (int)S, (int)Hq,
                      (int)Hkv, (int)D, cur_stream());
  return dqkv;
}

// ---------------- fused qkv split + QK RMSNorm + rope ----------------
struct QkvNormDims {
  int64_t B, S, Hq, Hkv, D;
};

// what both entry points require of the packed qkv, the two norm weights and
// the tables; `positions` is checked by rope_positions
QkvNormDims qkv_norm_check(const torch::Tensor& qkv, const torch::Tensor& wq,
                           const torch::Tensor& wk, const torch::Tensor& cos,
                           const torch::Tensor& sin, int64_t Hq, int64_t Hkv,
                           int64_t D) {
  CHECK_BF16_CONTIG(qkv);
  CHECK_BF16_CONTIG(wq);
  CHECK_BF16_CONTIG(wk);
  TORCH_CHECK(qkv.dim() == 3, "qkv_norm_rope expects qkv [B,S,W]");
  TORCH_CHECK(D == 64 || D == 128,
              "qkv_norm_rope: head dim must be 64 or 128, got ", D);
  TORCH_CHECK(Hq > 0 && Hkv > 0, "qkv_norm_rope: head counts must be positive");
  TORCH_CHECK(qkv.size(2) == (Hq + 2 * Hkv) * D,
              "qkv_norm_rope: packed width mismatch, W must be (Hq+2*Hkv)*D");
  TORCH_CHECK(wq.dim() == 1 && wq.size(0) == D && wk.dim() == 1 &&
                  wk.size(0) == D,
              "qkv_norm_rope: wq and wk must be [D]");
  TORCH_CHECK(wq.device() == qkv.device() && wk.device() == qkv.device(),
              "qkv_norm_rope: wq and wk must be on qkv's device");
  TORCH_CHECK(qkv.size(0) <= 65535 && qkv.size(1) <= INT32_MAX,
              "qkv_norm_rope: B must fit a grid dimension and S an int32");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(wq.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(wk.data_ptr()) % 16 == 0,
              "qkv_norm_rope: qkv, wq and wk must be 16-byte aligned");
  CHECK_ROPE_TABLES(cos, sin, qkv, D);
  return {qkv.size(0), qkv.size(1), Hq, Hkv, D};
}

std::vector<torch::Tensor> qkv_norm_rope_fwd(
    torch::Tensor qkv, torch::Tensor wq, torch::Tensor wk, torch::Tensor cos,
    torch::Tensor sin, c10::optional<torch::Tensor> positions, int64_t Hq,
    int64_t Hkv, int64_t D, double eps) {
  const QkvNormDims d = qkv_norm_check(qkv, wq, wk, cos, sin, Hq, Hkv, D);
  const int* pos_ptr = rope_positions(positions, cos, qkv, d.S);
  auto q = torch::empty({d.B, d.S, Hq, D}, qkv.options());
  auto k = torch::empty({d.B, d.S, Hkv, D}, qkv.options());
  auto v = torch::empty({d.B, d.S, Hkv, D}, qkv.options());
  qkv_norm_rope_fwd_launch(qkv.data_ptr(), wq.data_ptr(), wk.data_ptr(),
                           q.data_ptr(), k.data_ptr(), v.data_ptr(),
                           cos.data_ptr<float>(), sin.data_ptr<float>(),
                           pos_ptr, d.B, (int)d.S, (int)Hq, (int)Hkv, (int)D,
                           (float)eps, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {q, k, v};
}

// (dqkv [B,S,W], dwq [D], dwk [D]); dwq and dwk are the two halves of one
// [2*D] tensor
std::vector<torch::Tensor> qkv_norm_rope_bwd(
    torch::Tensor dq, torch::Tensor dk, torch::Tensor dv, torch::Tensor qkv,
    torch::Tensor wq, torch::Tensor wk, torch::Tensor cos, torch::Tensor sin,
    c10::optional<torch::Tensor> positions, double eps) {
  CHECK_BF16_CONTIG(dq);
  CHECK_BF16_CONTIG(dk);
  CHECK_BF16_CONTIG(dv);
  TORCH_CHECK(dq.dim() == 4, "dq must be [B,S,Hq,D]");
  TORCH_CHECK(dk.dim() == 4 && dk.size(0) == dq.size(0) &&
                  dk.size(1) == dq.size(1) && dk.size(3) == dq.size(3),
              "dk must be [B,S,Hkv,D]");
  TORCH_CHECK(dv.sizes() == dk.sizes(), "dv must be [B,S,Hkv,D]");
  TORCH_CHECK(dk.device() == dq.device() && dv.device() == dq.device() &&
                  qkv.device() == dq.device(),
              "dk, dv and qkv must be on dq's device");
  const int64_t Hq = dq.size(2), Hkv = dk.size(2), D = dq.size(3);
  const QkvNormDims d = qkv_norm_check(qkv, wq, wk, cos, sin, Hq, Hkv, D);
  TORCH_CHECK(d.B == dq.size(0) && d.S == dq.size(1),
              "qkv must be [B,S,W] with dq's B and S");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dq.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(dk.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(dv.data_ptr()) % 16 == 0,
              "qkv_norm_rope: dq, dk and dv must be 16-byte aligned");
  const int* pos_ptr = rope_positions(positions, cos, qkv, d.S);
  auto dqkv = torch::empty_like(qkv);
  if (d.B == 0 || d.S == 0) {
    auto dw0 = torch::zeros({2 * D}, wq.options());
    return {dqkv, dw0.narrow(0, 0, D), dw0.narrow(0, D, D)};
  }
  auto dw = torch::empty({2 * D}, wq.options());
  const int nblocks = qkv_norm_rope_bwd_blocks(d.B, (int)d.S);
  auto dw_partial = alloc_partials(nblocks, (int)(2 * D), qkv);
  qkv_norm_rope_bwd_launch(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                           qkv.data_ptr(), wq.data_ptr(), wk.data_ptr(),
                           dqkv.data_ptr(), dw_partial.data_ptr<float>(),
                           dw.data_ptr(), cos.data_ptr<float>(),
                           sin.data_ptr<float>(), pos_ptr, d.B, (int)d.S,
                           (int)Hq, (int)Hkv, (int)D, (float)eps,
                           cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dqkv, dw.narrow(0, 0, D), dw.narrow(0, D, D)};
}

// ---------------- mixture of experts (moe_router.hip, moe_dispatch.hip) ----
#define CHECK_ON_DEVICE_CONTIG(t, ref, type, what)                         \
  TORCH_CHECK((t).is_cuda() && (t).device() == (ref).device(),             \
              #t " must be on " #ref "'s device");                         \
  TORCH_CHECK((t).dtype() == (type) && (t).is_contiguous(),                \
              #t " must be contiguous " what)

// logits bf16 [T, E] with a supported E, and k in range for it
inline void moe_router_check(const torch::Tensor& logits, int64_t k) {
  CHECK_BF16_CONTIG(logits);
  TORCH_CHECK(logits.dim() == 2, "moe_router: logits must be [T, E]");
  const int64_t E = logits.size(1);
  TORCH_CHECK(E == 8 || E == 16 || E == 32 || E == 64 || E == 128,
              "moe_router: E must be 8, 16, 32, 64 or 128, got ", E);
  TORCH_CHECK(k >= 1 && k <= 8 && k <= E,
              "moe_router: k must be in [1, min(8, E)], got ", k);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 4 == 0,
              "moe_router: logits must be 4-byte aligned");
}

std::vector<torch::Tensor> moe_router_fwd(torch::Tensor logits, int64_t k,
                                          bool norm) {
  moe_router_check(logits, k);
  const int64_t T = logits.size(0), E = logits.size(1);
  auto idx = torch::empty({T, k}, logits.options().dtype(torch::kInt));
  auto w = torch::empty({T, k}, logits.options().dtype(torch::kFloat));
  moe_router_fwd_launch(logits.data_ptr(), idx.data_ptr<int>(),
                        w.data_ptr<float>(), T, (int)E, (int)k, norm ? 1 : 0,
                        cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {idx, w};
}

torch::Tensor moe_router_bwd(torch::Tensor logits, torch::Tensor topk_idx,
                             torch::Tensor d_topk_w, bool norm) {
  TORCH_CHECK(topk_idx.dim() == 2, "topk_idx must be [T, k]");
  const int64_t k = topk_idx.size(1);
  moe_router_check(logits, k);
  const int64_t T = logits.size(0), E = logits.size(1);
  CHECK_ON_DEVICE_CONTIG(topk_idx, logits, torch::kInt, "int32");
  CHECK_ON_DEVICE_CONTIG(d_topk_w, logits, torch::kFloat, "f32");
  TORCH_CHECK(topk_idx.size(0) == T && d_topk_w.sizes() == topk_idx.sizes(),
              "topk_idx and d_topk_w must be [T, k] with the logits' T");
  auto dlogits = torch::empty_like(logits);
  moe_router_bwd_launch(logits.data_ptr(), topk_idx.data_ptr<int>(),
                        d_topk_w.data_ptr<float>(), dlogits.data_ptr(), T,
                        (int)E, (int)k, norm ? 1 : 0, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dlogits;
}

// (topk_idx, topk_w, counts int32 [E], aux, z): the router with the
// load-balancing loss and the z-loss of its T >= 1 tokens as 0-dim f32
std::vector<torch::Tensor> moe_router_aux_fwd(torch::Tensor logits, int64_t k,
                                              bool norm) {
  moe_router_check(logits, k);
  const int64_t T = logits.size(0), E = logits.size(1);
  TORCH_CHECK(T >= 1 && T <= INT32_MAX,
              "moe_router_aux: T must be in [1, 2^31), got ", T);
  auto idx = torch::empty({T, k}, logits.options().dtype(torch::kInt));
  auto fopt = logits.options().dtype(torch::kFloat);
  auto w = torch::empty({T, k}, fopt);
  auto counts = torch::empty({E}, logits.options().dtype(torch::kInt));
  auto aux = torch::empty({}, fopt);
  auto z = torch::empty({}, fopt);
  auto partials =
      torch::empty({moe_router_aux_grid(T, (int)E), 2 * E + 1}, fopt);
  moe_router_aux_fwd_launch(logits.data_ptr(), idx.data_ptr<int>(),
                            w.data_ptr<float>(), partials.data_ptr<float>(),
                            counts.data_ptr<int>(), aux.data_ptr<float>(),
                            z.data_ptr<float>(), T, (int)E, (int)k,
                            norm ? 1 : 0, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {idx, w, counts, aux, z};
}

torch::Tensor moe_router_aux_bwd(torch::Tensor logits, torch::Tensor topk_idx,
                                 torch::Tensor d_topk_w, torch::Tensor counts,
                                 torch::Tensor g_aux, torch::Tensor g_z,
                                 bool norm) {
  TORCH_CHECK(topk_idx.dim() == 2, "topk_idx must be [T, k]");
  const int64_t k = topk_idx.size(1);
  moe_router_check(logits, k);
  const int64_t T = logits.size(0), E = logits.size(1);
  CHECK_ON_DEVICE_CONTIG(topk_idx, logits, torch::kInt, "int32");
  CHECK_ON_DEVICE_CONTIG(d_topk_w, logits, torch::kFloat, "f32");
  CHECK_ON_DEVICE_CONTIG(counts, logits, torch::kInt, "int32");
  CHECK_ON_DEVICE_CONTIG(g_aux, logits, torch::kFloat, "f32");
  CHECK_ON_DEVICE_CONTIG(g_z, logits, torch::kFloat, "f32");
  TORCH_CHECK(topk_idx.size(0) == T && d_topk_w.sizes() == topk_idx.sizes(),
              "topk_idx and d_topk_w must be [T, k] with the logits' T");
  TORCH_CHECK(counts.dim() == 1 && counts.size(0) == E,
              "counts must be [E]");
  TORCH_CHECK(g_aux.numel() == 1 && g_z.numel() == 1,
              "g_aux and g_z must hold one element each");
  auto dlogits = torch::empty_like(logits);
  moe_router_aux_bwd_launch(logits.data_ptr(), topk_idx.data_ptr<int>(),
                            d_topk_w.data_ptr<float>(),
                            counts.data_ptr<int>(), g_aux.data_ptr<float>(),
                            g_z.data_ptr<float>(), dlogits.data_ptr(), T,
                            (int)E, (int)k, norm ? 1 : 0, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dlogits;
}

// (dest [T*k], offs [E]): views of one int32 buffer whose tail is the index
// build's scratch
std::vector<torch::Tensor> moe_dispatch_index(torch::Tensor topk_idx,
                                              int64_t E) {
  TORCH_CHECK(topk_idx.is_cuda(), "topk_idx must be on the GPU");
  TORCH_CHECK(topk_idx.dtype() == torch::kInt && topk_idx.is_contiguous(),
              "topk_idx must be contiguous int32");
  TORCH_CHECK(topk_idx.dim() == 2, "topk_idx must be [T, k]");
  TORCH_CHECK(E == 8 || E == 16 || E == 32 || E == 64 || E == 128,
              "moe_dispatch_index: E must be 8, 16, 32, 64 or 128, got ", E);
  const int64_t N = topk_idx.numel();
  TORCH_CHECK(N <= INT32_MAX, "moe_dispatch_index: T*k must fit an int32");
  auto buf = torch::empty({N + E + moe_index_scratch(N, (int)E)},
                          topk_idx.options());
  int* p = buf.data_ptr<int>();
  moe_index_launch(topk_idx.data_ptr<int>(), p, p + N, p + N + E, N, (int)E,
                   cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {buf.narrow(0, 0, N), buf.narrow(0, N, E)};
}

// what the row movers require: rows bf16 [R, H] with H % 8 == 0, dest int32
// [N] on the rows' device; moe_k_check then derives k = N / T
inline void moe_rows_check(const torch::Tensor& rows, const torch::Tensor& dest,
                           const char* what) {
  CHECK_BF16_CONTIG(rows);
  TORCH_CHECK(rows.dim() == 2, what, ": rows must be [R, H]");
  TORCH_CHECK(rows.size(1) > 0 && rows.size(1) % 8 == 0 &&
                  rows.size(1) <= INT32_MAX,
              what, ": H must be a positive multiple of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(rows.data_ptr()) % 16 == 0, what,
              ": rows must be 16-byte aligned");
  CHECK_ON_DEVICE_CONTIG(dest, rows, torch::kInt, "int32");
  TORCH_CHECK(dest.dim() == 1, what, ": dest must be [T*k]");
}

inline int64_t moe_k_check(int64_t T, int64_t N, const char* what) {
  TORCH_CHECK(N == 0 ? T == 0 : (T > 0 && N % T == 0 && N / T <= 8), what,
              ": dest must hold k <= 8 slots per token");
  return T == 0 ? 1 : N / T;
}

// xp [T*k, H]: a copy of x[t] at every row dest[t*k + j]
torch::Tensor moe_scatter(torch::Tensor x, torch::Tensor dest) {
  moe_rows_check(x, dest, "moe_scatter");
  const int64_t T = x.size(0), H = x.size(1), N = dest.numel();
  const int64_t k = moe_k_check(T, N, "moe_scatter");
  auto xp = torch::empty({N, H}, x.options());
  moe_scatter_launch(x.data_ptr(), dest.data_ptr<int>(), nullptr, nullptr,
                     xp.data_ptr(), nullptr, T, (int)H, (int)k, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return xp;
}

// y [T, H] = sum_j w[t, j] * yp[dest[t*k + j]]; without w the weights are 1
torch::Tensor moe_combine(torch::Tensor yp, torch::Tensor dest,
                          c10::optional<torch::Tensor> w, int64_t k) {
  moe_rows_check(yp, dest, "moe_combine");
  const int64_t N = dest.numel(), H = yp.size(1);
  TORCH_CHECK(yp.size(0) == N, "moe_combine: yp must be [T*k, H]");
  TORCH_CHECK(k >= 1 && k <= 8 && N % k == 0,
              "moe_combine: k must be in [1, 8] and divide dest's length");
  const int64_t T = N / k;
  const float* wp = nullptr;
  if (w.has_value()) {
    CHECK_ON_DEVICE_CONTIG(*w, yp, torch::kFloat, "f32");
    TORCH_CHECK(w->dim() == 2 && w->size(0) == T && w->size(1) == k,
                "moe_combine: w must be [T, k]");
    wp = w->data_ptr<float>();
  }
  auto y = torch::empty({T, H}, yp.options());
  moe_combine_launch(yp.data_ptr(), dest.data_ptr<int>(), wp, y.data_ptr(), T,
                     (int)H, (int)k, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return y;
}

// the combine's backward: (dyp [T*k, H], dw [T, k])
std::vector<torch::Tensor> moe_combine_bwd(torch::Tensor dy,
                                           torch::Tensor dest,
                                           torch::Tensor w,
                                           torch::Tensor yp) {
  moe_rows_check(dy, dest, "moe_combine_bwd");
  moe_rows_check(yp, dest, "moe_combine_bwd");
  const int64_t T = dy.size(0), H = dy.size(1), N = dest.numel();
  CHECK_ON_DEVICE_CONTIG(w, dy, torch::kFloat, "f32");
  TORCH_CHECK(w.dim() == 2 && w.size(0) == T && w.numel() == N,
              "moe_combine_bwd: w must be [T, k]");
  const int64_t k = moe_k_check(T, N, "moe_combine_bwd");
  TORCH_CHECK(yp.size(0) == N && yp.size(1) == H,
              "moe_combine_bwd: yp must be [T*k, H]");
  auto dyp = torch::empty_like(yp);
  auto dw = torch::empty_like(w);
  moe_scatter_launch(dy.data_ptr(), dest.data_ptr<int>(), w.data_ptr<float>(),
                     yp.data_ptr(), dyp.data_ptr(), dw.data_ptr<float>(), T,
                     (int)H, (int)k, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dyp, dw};
}

// ---------------- expert GEMMs (moe_gemm.hip) ----------------
// rows bf16 [N, inner], weight bf16 [E, M, K], offs int32 [E]: the contract
// of ops/moe.py's moe_gemm_supported, checked again here
inline void moe_gemm_check(const torch::Tensor& rows, int64_t E, int64_t M,
                           int64_t K, const torch::Tensor& offs,
                           const char* what) {
  CHECK_BF16_CONTIG(rows);
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) <= INT32_MAX - 256, what,
              ": rows must be [N, .] with N < 2^31 - 256");
  TORCH_CHECK(E >= 1 && E <= 128, what, ": E must be in [1, 128], got ", E);
  TORCH_CHECK(M >= 64 && M % 64 == 0 && K >= 64 && K % 64 == 0 &&
                  E * M * K <= INT64_MAX / 4 && M <= (1 << 24) &&
                  K <= (1 << 24),
              what, ": M and K must be positive multiples of 64, got ", M,
              ", ", K);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(rows.data_ptr()) % 16 == 0, what,
              ": rows must be 16-byte aligned");
  CHECK_ON_DEVICE_CONTIG(offs, rows, torch::kInt, "int32");
  TORCH_CHECK(offs.dim() == 1 && offs.size(0) == E, what,
              ": offs must be [E]");
}

// trans_b false: y [N, M] = a [N, K] . weight[e]^T; true: da [N, K] =
// a (= dy) [N, M] . weight[e], per expert group of rows
torch::Tensor moe_gemm_rows(torch::Tensor a, torch::Tensor weight,
                            torch::Tensor offs, bool trans_b) {
  TORCH_CHECK(weight.dim() == 3, "moe_gemm_rows: weight must be [E, M, K]");
  const int64_t E = weight.size(0), M = weight.size(1), K = weight.size(2);
  moe_gemm_check(a, E, M, K, offs, "moe_gemm_rows");
  CHECK_ON_DEVICE_CONTIG(weight, a, torch::kBFloat16, "bf16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0,
              "moe_gemm_rows: weight must be 16-byte aligned");
  TORCH_CHECK(a.size(1) == (trans_b ? M : K),
              "moe_gemm_rows: rows' width must be weight's ",
              trans_b ? "M" : "K");
  const int64_t N = a.size(0);
  TORCH_CHECK((N / 128 + 1 + E) * ((M > K ? M : K) / 128 + 1) <= INT32_MAX,
              "moe_gemm_rows: too many tiles for one grid");
  auto out = torch::empty({N, trans_b ? K : M}, a.options());
  moe_gemm_rows_launch(a.data_ptr(), weight.data_ptr(), offs.data_ptr<int>(),
                       out.data_ptr(), N, (int)E, (int)M, (int)K,
                       trans_b ? 1 : 0, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// dw [E, M, K] = dy[rows of e]^T . a[rows of e]
torch::Tensor moe_gemm_dw(torch::Tensor dy, torch::Tensor a,
                          torch::Tensor offs) {
  TORCH_CHECK(dy.dim() == 2 && a.dim() == 2 && dy.size(0) == a.size(0),
              "moe_gemm_dw: dy [N, M] and a [N, K]");
  const int64_t E = offs.numel(), M = dy.size(1), K = a.size(1);
  moe_gemm_check(dy, E, M, K, offs, "moe_gemm_dw");
  moe_gemm_check(a, E, M, K, offs, "moe_gemm_dw");
  TORCH_CHECK(E * (M / 128 + 1) * (K / 128 + 1) <= INT32_MAX,
              "moe_gemm_dw: too many tiles for one grid");
  auto dw = torch::empty({E, M, K}, a.options());
  moe_gemm_dw_launch(dy.data_ptr(), a.data_ptr(), offs.data_ptr<int>(),
                     dw.data_ptr(), a.size(0), (int)E, (int)M, (int)K,
                     cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dw;
}

// ---------------- gather-fused expert GEMMs (moe_gemm_gather.hip) ---------
// row_src int32 [T*k]: the token of every row of the expert-sorted layout
torch::Tensor moe_row_src(torch::Tensor dest, int64_t k) {
  TORCH_CHECK(dest.is_cuda() && dest.dtype() == torch::kInt &&
                  dest.is_contiguous() && dest.dim() == 1,
              "moe_row_src: dest must be contiguous int32 [T*k] on the GPU");
  const int64_t N = dest.numel();
  TORCH_CHECK(k >= 1 && k <= 8 && N % k == 0 && N <= INT32_MAX,
              "moe_row_src: k must be in [1, 8] and divide dest's length");
  auto row_src = torch::empty({N}, dest.options());
  moe_row_src_launch(dest.data_ptr<int>(), row_src.data_ptr<int>(), N / k,
                     (int)k, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return row_src;
}

// x [T, K] with T >= 1 wherever there is a row; row_src int32 [N]
inline void moe_gather_check(const torch::Tensor& x,
                             const torch::Tensor& row_src, int64_t E,
                             int64_t M, int64_t K, const torch::Tensor& offs,
                             const char* what) {
  moe_gemm_check(x, E, M, K, offs, what);
  TORCH_CHECK(x.size(1) == K, what, ": x must be [T, K]");
  CHECK_ON_DEVICE_CONTIG(row_src, x, torch::kInt, "int32");
  TORCH_CHECK(row_src.dim() == 1 && row_src.numel() <= INT32_MAX - 256, what,
              ": row_src must be [N] with N < 2^31 - 256");
  TORCH_CHECK(row_src.numel() == 0 || x.size(0) > 0, what,
              ": rows without a token to read");
}

// y [N, M] = x[row_src[r]] . weight[e]^T per expert group of rows
torch::Tensor moe_gemm_rows_gather(torch::Tensor x, torch::Tensor row_src,
                                   torch::Tensor weight, torch::Tensor offs) {
  TORCH_CHECK(weight.dim() == 3,
              "moe_gemm_rows_gather: weight must be [E, M, K]");
  const int64_t E = weight.size(0), M = weight.size(1), K = weight.size(2);
  moe_gather_check(x, row_src, E, M, K, offs, "moe_gemm_rows_gather");
  CHECK_ON_DEVICE_CONTIG(weight, x, torch::kBFloat16, "bf16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(weight.data_ptr()) % 16 == 0,
              "moe_gemm_rows_gather: weight must be 16-byte aligned");
  const int64_t N = row_src.numel();
  TORCH_CHECK((N / 128 + 1 + E) * (M / 128 + 1) <= INT32_MAX,
              "moe_gemm_rows_gather: too many tiles for one grid");
  auto out = torch::empty({N, M}, x.options());
  moe_gemm_rows_gather_launch(x.data_ptr(), row_src.data_ptr<int>(),
                              weight.data_ptr(), offs.data_ptr<int>(),
                              out.data_ptr(), N, x.size(0), (int)E, (int)M,
                              (int)K, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// dw [E, M, K] = dy[rows of e]^T . x[row_src[rows of e]]
torch::Tensor moe_gemm_dw_gather(torch::Tensor dy, torch::Tensor x,
                                 torch::Tensor row_src, torch::Tensor offs) {
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 &&
                  dy.size(0) == row_src.numel(),
              "moe_gemm_dw_gather: dy [N, M], x [T, K], row_src [N]");
  const int64_t E = offs.numel(), M = dy.size(1), K = x.size(1);
  moe_gemm_check(dy, E, M, K, offs, "moe_gemm_dw_gather");
  moe_gather_check(x, row_src, E, M, K, offs, "moe_gemm_dw_gather");
  TORCH_CHECK(E * (M / 128 + 1) * (K / 128 + 1) <= INT32_MAX,
              "moe_gemm_dw_gather: too many tiles for one grid");
  auto dw = torch::empty({E, M, K}, x.options());
  moe_gemm_dw_gather_launch(dy.data_ptr(), x.data_ptr(),
                            row_src.data_ptr<int>(), offs.data_ptr<int>(),
                            dw.data_ptr(), dy.size(0), x.size(0), (int)E,
                            (int)M, (int)K, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dw;
}

// ---------------- weighted-SwiGLU expert GEMMs (moe_gemm_swiglu.hip) -------
// w_row f32 [T*k]: the router weight of every row of the expert-sorted layout
torch::Tensor moe_row_w(torch::Tensor dest, torch::Tensor topk_w) {
  TORCH_CHECK(dest.is_cuda() && dest.dtype() == torch::kInt &&
                  dest.is_contiguous() && dest.dim() == 1,
              "moe_row_w: dest must be contiguous int32 [T*k] on the GPU");
  CHECK_ON_DEVICE_CONTIG(topk_w, dest, torch::kFloat, "f32");
  const int64_t N = dest.numel();
  TORCH_CHECK(topk_w.dim() == 2 && topk_w.numel() == N &&
                  topk_w.size(1) >= 1 && topk_w.size(1) <= 8 &&
                  N <= INT32_MAX,
              "moe_row_w: topk_w must be [T, k] with k in [1, 8], dest [T*k]");
  auto w_row = torch::empty({N}, topk_w.options());
  moe_row_w_launch(dest.data_ptr<int>(), topk_w.data_ptr<float>(),
                   w_row.data_ptr<float>(), topk_w.size(0),
                   (int)topk_w.size(1), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return w_row;
}

// (gu [N, 2I], h' [N, I]) of gate_up [E, 2I, K] on x [T, K] through row_src
std::vector<torch::Tensor> moe_gemm_gu_swiglu(torch::Tensor x,
                                              torch::Tensor row_src,
                                              torch::Tensor w_row,
                                              torch::Tensor gate_up,
                                              torch::Tensor offs) {
  TORCH_CHECK(gate_up.dim() == 3,
              "moe_gemm_gu_swiglu: gate_up must be [E, 2I, K]");
  const int64_t E = gate_up.size(0), M = gate_up.size(1), K = gate_up.size(2);
  moe_gather_check(x, row_src, E, M, K, offs, "moe_gemm_gu_swiglu");
  TORCH_CHECK(M % 128 == 0, "moe_gemm_gu_swiglu: I must be a multiple of 64");
  CHECK_ON_DEVICE_CONTIG(gate_up, x, torch::kBFloat16, "bf16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(gate_up.data_ptr()) % 16 == 0,
              "moe_gemm_gu_swiglu: gate_up must be 16-byte aligned");
  const int64_t N = row_src.numel(), I = M / 2;
  CHECK_ON_DEVICE_CONTIG(w_row, x, torch::kFloat, "f32");
  TORCH_CHECK(w_row.dim() == 1 && w_row.numel() == N,
              "moe_gemm_gu_swiglu: w_row must be [N]");
  TORCH_CHECK((N / 128 + 1 + E) * (I / 64) <= INT32_MAX,
              "moe_gemm_gu_swiglu: too many tiles for one grid");
  auto gu = torch::empty({N, M}, x.options());
  auto hw = torch::empty({N, I}, x.options());
  moe_gemm_gu_swiglu_launch(x.data_ptr(), row_src.data_ptr<int>(),
                            w_row.data_ptr<float>(), gate_up.data_ptr(),
                            offs.data_ptr<int>(), gu.data_ptr(), hw.data_ptr(),
                            N, x.size(0), (int)E, (int)I, (int)K,
                            cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {gu, hw};
}

// (dgu [N, 2I], dw_topk f32 [N]) from dyp [N, H], down [E, H, I], the saved
// gu [N, 2I], w_row [N] and dest [N]
std::vector<torch::Tensor> moe_gemm_da_swiglu(torch::Tensor dyp,
                                              torch::Tensor down,
                                              torch::Tensor gu,
                                              torch::Tensor w_row,
                                              torch::Tensor offs,
                                              torch::Tensor dest) {
  TORCH_CHECK(down.dim() == 3, "moe_gemm_da_swiglu: down must be [E, H, I]");
  const int64_t E = down.size(0), H = down.size(1), I = down.size(2);
  moe_gemm_check(dyp, E, H, I, offs, "moe_gemm_da_swiglu");
  moe_gemm_check(gu, E, H, I, offs, "moe_gemm_da_swiglu");
  CHECK_ON_DEVICE_CONTIG(down, dyp, torch::kBFloat16, "bf16");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(down.data_ptr()) % 16 == 0,
              "moe_gemm_da_swiglu: down must be 16-byte aligned");
  const int64_t N = dyp.size(0);
  TORCH_CHECK(dyp.size(1) == H && gu.size(0) == N && gu.size(1) == 2 * I &&
                  gu.device() == dyp.device(),
              "moe_gemm_da_swiglu: dyp [N, H] and gu [N, 2I]");
  CHECK_ON_DEVICE_CONTIG(w_row, dyp, torch::kFloat, "f32");
  CHECK_ON_DEVICE_CONTIG(dest, dyp, torch::kInt, "int32");
  TORCH_CHECK(w_row.dim() == 1 && w_row.numel() == N && dest.dim() == 1 &&
                  dest.numel() == N,
              "moe_gemm_da_swiglu: w_row and dest must be [N]");
  TORCH_CHECK((N / 128 + 1 + E) * (I / 128 + 1) <= INT32_MAX,
              "moe_gemm_da_swiglu: too many tiles for one grid");
  auto dgu = torch::empty_like(gu);
  auto dwp = torch::empty({N, moe_dw_parts((int)I)}, w_row.options());
  auto dw = torch::empty({N}, w_row.options());
  moe_gemm_da_swiglu_launch(dyp.data_ptr(), down.data_ptr(), gu.data_ptr(),
                            w_row.data_ptr<float>(), offs.data_ptr<int>(),
                            dest.data_ptr<int>(), dgu.data_ptr(),
                            dwp.data_ptr<float>(), dw.data_ptr<float>(), N,
                            (int)E, (int)H, (int)I, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dgu, dw};
}

// ---------------- silu_mul ----------------
torch::Tensor silu_mul_fwd(torch::Tensor gu) {
  CHECK_BF16_CONTIG(gu);
  const int I2 = (int)gu.size(-1);
  TORCH_CHECK(I2 % 16 == 0, "packed gate_up dim must be a multiple of 16");
  const int I = I2 / 2;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto y = torch::empty(sizes, gu.options());
  silu_mul_fwd_launch(gu.data_ptr(), y.data_ptr(), gu.numel() / I2, I,
                      cur_stream());
  return y;
}

torch::Tensor silu_mul_bwd(torch::Tensor dy, torch::Tensor gu) {
  CHECK_BF16_CONTIG(dy);
  CHECK_BF16_CONTIG(gu);
  const int I2 = (int)gu.size(-1);
  TORCH_CHECK(I2 % 16 == 0, "packed gate_up dim must be a multiple of 16");
  const int I = I2 / 2;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  TORCH_CHECK(dy.sizes() == c10::IntArrayRef(sizes),
              "dy must have gu's shape with the last dim halved");
  TORCH_CHECK(dy.device() == gu.device(), "dy must be on gu's device");
  auto dgu = torch::empty_like(gu);
  silu_mul_bwd_launch(dy.data_ptr(), gu.data_ptr(), dgu.data_ptr(),
                      gu.numel() / I2, I, cur_stream());
  return dgu;
}

// ---------------- embedding ----------------
torch::Tensor embedding_fwd(torch::Tensor table, torch::Tensor ids) {
  CHECK_BF16_CONTIG(table);
  TORCH_CHECK(table.dim() == 2, "table must be [V,H]");
  TORCH_CHECK(ids.is_cuda() && ids.device() == table.device(),
              "ids must be on the table's device");
  TORCH_CHECK(ids.dtype() == torch::kLong && ids.is_contiguous());
  const int64_t V = table.size(0);
  const int H = (int)table.size(1);
  auto sizes = ids.sizes().vec();
  sizes.push_back(H);
  auto out = torch::empty(sizes, table.options());
  embed_fwd_launch(table.data_ptr(), ids.data_ptr<int64_t>(),
                   out.data_ptr(), ids.numel(), H, V, cur_stream());
  return out;
}

torch::Tensor embedding_bwd(torch::Tensor dy, torch::Tensor ids, int64_t V) {
  CHECK_BF16_CONTIG(dy);
  TORCH_CHECK(ids.is_cuda() && ids.device() == dy.device(),
              "ids must be on dy's device");
  TORCH_CHECK(ids.dtype() == torch::kLong && ids.is_contiguous());
  TORCH_CHECK(dy.dim() >= 1 && V > 0, "dy must be [..., H] and V positive");
  const int H = (int)dy.size(-1);
  TORCH_CHECK(dy.numel() == ids.numel() * H, "dy/ids shape mismatch");
  auto acc = torch::empty({V, (int64_t)H},
                          dy.options().dtype(torch::kFloat));
  auto dtable = torch::empty({V, (int64_t)H}, dy.options());
  embed_bwd_launch(dy.data_ptr(), ids.data_ptr<int64_t>(),
                   acc.data_ptr<float>(), dtable.data_ptr(), ids.numel(), H,
                   V, cur_stream());
  return dtable;
}

// the atomic-free form: its scratch is O(N) + O(V) ints and N / 128 f32 rows
torch::Tensor embedding_bwd_sorted(torch::Tensor dy, torch::Tensor ids,
                                   int64_t V) {
  CHECK_BF16_CONTIG(dy);
  TORCH_CHECK(ids.is_cuda() && ids.device() == dy.device(),
              "ids must be on dy's device");
  TORCH_CHECK(ids.dtype() == torch::kLong && ids.is_contiguous());
  TORCH_CHECK(dy.dim() >= 1 && V > 0, "dy must be [..., H] and V positive");
  const int H = (int)dy.size(-1);
  TORCH_CHECK(dy.numel() == ids.numel() * H, "dy/ids shape mismatch");
  const int64_t N = ids.numel();
  TORCH_CHECK(N < INT32_MAX - 1024 && V <= ((int64_t)1 << 30),
              "embedding_bwd_sorted: ids.numel() and V must fit an int32");
  auto scratch = torch::empty({embed_bwd_sorted_scratch(N, V)},
                              dy.options().dtype(torch::kInt));
  auto partials = torch::empty({embed_bwd_sorted_partials(N), (int64_t)H},
                               dy.options().dtype(torch::kFloat));
  auto dtable = torch::empty({V, (int64_t)H}, dy.options());
  embed_bwd_sorted_launch(dy.data_ptr(), ids.data_ptr<int64_t>(),
                          scratch.data_ptr<int>(), partials.data_ptr<float>(),
                          dtable.data_ptr(), N, H, V, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dtable;
}

// ---------------- gelu (GPT-2 MLP) ----------------
torch::Tensor gelu_fwd(torch::Tensor x) {
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(x.numel() % 8 == 0, "gelu kernel needs numel % 8 == 0");
  auto y = torch::empty_like(x);
  gelu_fwd_launch(x.data_ptr(), y.data_ptr(), x.numel(), cur_stream());
  return y;
}

torch::Tensor gelu_bwd(torch::Tensor dy, torch::Tensor x) {
  CHECK_BF16_CONTIG(dy);
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(dy.numel() == x.numel(), "gelu_bwd: dy/x numel mismatch");
  TORCH_CHECK(dy.device() == x.device(), "dy must be on x's device");
  TORCH_CHECK(x.numel() % 8 == 0, "gelu kernel needs numel % 8 == 0");
  auto dx = torch::empty_like(x);
  gelu_bwd_launch(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(),
                  cur_stream());
  return dx;
}

// ---------------- cross entropy ----------------
std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor labels,
                                  int64_t S_out, int64_t ignore_index) {
  CHECK_CE_INPUTS(logits, labels, S_out);
  const int B = (int)logits.size(0), S = (int)logits.size(1),
            V = (int)logits.size(2);
  const int64_t nrows = (int64_t)B * S_out;
  auto loss = torch::empty({nrows}, logits.options().dtype(torch::kFloat));
  auto lse = torch::empty({nrows}, logits.options().dtype(torch::kFloat));
  ce_fwd_launch(logits.data_ptr(), labels.data_ptr<int64_t>(),
                loss.data_ptr<float>(), lse.data_ptr<float>(), nrows, S,
                (int)S_out, V, ignore_index, cur_stream());
  return {loss, lse};
}

std::vector<torch::Tensor> ce_fwd_sharded(torch::Tensor logits,
                                          torch::Tensor labels, int64_t S_out,
                                          int64_t vocab_start,
                                          int64_t ignore_index) {
  CHECK_CE_INPUTS(logits, labels, S_out);
  const int B = (int)logits.size(0), S = (int)logits.size(1),
            V = (int)logits.size(2);
  const int64_t nrows = (int64_t)B * S_out;
  auto opts = logits.options().dtype(torch::kFloat);
  auto maxout = torch::empty({nrows}, opts);
  auto sumout = torch::empty({nrows}, opts);
  auto gathered = torch::empty({nrows}, opts);
  ce_fwd_sharded_launch(logits.data_ptr(), labels.data_ptr<int64_t>(),
                        maxout.data_ptr<float>(), sumout.data_ptr<float>(),
                        gathered.data_ptr<float>(), nrows, S, (int)S_out, V,
                        vocab_start, ignore_index, cur_stream());
  return {maxout, sumout, gathered};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor labels,
                     torch::Tensor lse, double scale, int64_t S_out,
                     int64_t vocab_start, int64_t ignore_index, bool sharded,
                     c10::optional<torch::Tensor> scale_t = c10::nullopt) {
  CHECK_CE_INPUTS(logits, labels, S_out);
  const int B = (int)logits.size(0), S = (int)logits.size(1),
            V = (int)logits.size(2);
  const int64_t nrows = (int64_t)B * S_out;
  TORCH_CHECK(lse.is_cuda() && lse.device() == logits.device() &&
                  lse.dtype() == torch::kFloat && lse.is_contiguous() &&
                  lse.numel() == nrows,
              "lse must be a contiguous f32 [B*S_out] on the logits' device");
  const float* sp = nullptr;
  if (scale_t.has_value()) {
    TORCH_CHECK(scale_t->dtype() == torch::kFloat && scale_t->is_cuda() &&
                scale_t->numel() == 1, "scale_t must be a cuda f32 scalar");
    sp = scale_t->data_ptr<float>();
  }
  // all rows with S_out == S are loss rows (the kernel writes every one);
  // otherwise the skipped rows must stay zero
  auto dlogits = (S_out == S) ? torch::empty_like(logits)
                              : torch::zeros_like(logits);
  ce_bwd_launch(logits.data_ptr(), labels.data_ptr<int64_t>(),
                lse.data_ptr<float>(), dlogits.data_ptr(), (float)scale, sp,
                nrows, S, (int)S_out, V, vocab_start, ignore_index,
                sharded ? 1 : 0, cur_stream());
  return dlogits;
}

// ---------------- adamw ----------------
void adamw_step(torch::Tensor descs, int64_t nchunks, double lr, double beta1,
                double beta2, double eps, double wd, int64_t step) {
  TORCH_CHECK(descs.is_cuda() && descs.dtype() == torch::kLong &&
              descs.is_contiguous());
  const float bc1 = 1.0f - std::pow((float)beta1, (float)step);
  const float bc2 = 1.0f - std::pow((float)beta2, (float)step);
  adamw_launch(descs.data_ptr(), (int)nchunks, (float)lr, (float)beta1,
               (float)beta2, (float)eps, (float)wd, 1.0f / bc1, 1.0f / bc2,
               cur_stream());
}

#define CHECK_DESCS(descs, nchunks)                                        \
  TORCH_CHECK((descs).is_cuda() && (descs).dtype() == torch::kLong &&      \
              (descs).is_contiguous());                                    \
  TORCH_CHECK((nchunks) >= 0 && (descs).numel() >= 7 * (nchunks),          \
              "descriptor table shorter than nchunks")

#define CHECK_SQ_TOTAL(t, descs)                                           \
  TORCH_CHECK((t).is_cuda() && (t).dtype() == torch::kFloat &&             \
              (t).numel() == 1 && (t).device() == (descs).device(),        \
              #t " must be a cuda f32 scalar on the descriptors' device")

void adamw_step_clipped(torch::Tensor descs, int64_t nchunks, double lr,
                        double beta1, double beta2, double eps, double wd,
                        int64_t step, torch::Tensor sq_total,
                        double max_norm) {
  CHECK_DESCS(descs, nchunks);
  CHECK_SQ_TOTAL(sq_total, descs);
  const float bc1 = 1.0f - std::pow((float)beta1, (float)step);
  const float bc2 = 1.0f - std::pow((float)beta2, (float)step);
  adamw_launch_clipped(descs.data_ptr(), (int)nchunks, (float)lr,
                       (float)beta1, (float)beta2, (float)eps, (float)wd,
                       1.0f / bc1, 1.0f / bc2, sq_total.data_ptr<float>(),
                       (float)max_norm, cur_stream());
}

// master-weight form (adamw.hip MASTER instantiations): lo_ptrs is the
// [nchunks] int64 table of companion pointers, sq_total absent = unclipped
void adamw_master_step(torch::Tensor descs, torch::Tensor lo_ptrs,
                       int64_t nchunks, double lr, double beta1, double beta2,
                       double eps, double wd, int64_t step,
                       c10::optional<torch::Tensor> sq_total,
                       double max_norm) {
  CHECK_DESCS(descs, nchunks);
  TORCH_CHECK(lo_ptrs.is_cuda() && lo_ptrs.dtype() == torch::kLong &&
              lo_ptrs.is_contiguous() && lo_ptrs.numel() >= nchunks &&
              lo_ptrs.device() == descs.device(),
              "lo_ptrs must be a cuda int64 table of >= nchunks pointers on "
              "the descriptors' device");
  const float* sq = nullptr;
  if (sq_total.has_value()) {
    CHECK_SQ_TOTAL(*sq_total, descs);
    sq = sq_total->data_ptr<float>();
  }
  const float bc1 = 1.0f - std::pow((float)beta1, (float)step);
  const float bc2 = 1.0f - std::pow((float)beta2, (float)step);
  adamw_master_launch(descs.data_ptr(), lo_ptrs.data_ptr<int64_t>(),
                      (int)nchunks, (float)lr, (float)beta1, (float)beta2,
                      (float)eps, (float)wd, 1.0f / bc1, 1.0f / bc2, sq,
                      (float)max_norm, cur_stream());
}

// ---------------- global grad norm / clipping ----------------
void grad_sqsum(torch::Tensor descs, int64_t nchunks, torch::Tensor partials,
                torch::Tensor out, int64_t slot) {
  CHECK_DESCS(descs, nchunks);
  TORCH_CHECK(partials.is_cuda() && partials.dtype() == torch::kFloat &&
              partials.is_contiguous() && partials.numel() >= nchunks &&
              partials.device() == descs.device(),
              "partials must be a cuda f32 buffer of >= nchunks elements");
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat &&
              out.is_contiguous() && out.device() == descs.device() &&
              slot >= 0 && slot < out.numel(),
              "out must be a cuda f32 buffer holding `slot`");
  grad_sqsum_launch(descs.data_ptr(), (int)nchunks,
                    partials.data_ptr<float>(), out.data_ptr<float>(),
                    (int)slot, cur_stream());
}

void grad_scale_(torch::Tensor descs, int64_t nchunks, torch::Tensor sq_total,
                 double max_norm) {
  CHECK_DESCS(descs, nchunks);
  CHECK_SQ_TOTAL(sq_total, descs);
  grad_scale_launch(descs.data_ptr(), (int)nchunks,
                    sq_total.data_ptr<float>(), (float)max_norm,
                    cur_stream());
}

// ---------------- fp8 quantisation (fp8_quant.hip) ----------------
// x: bf16 [R, C] on the GPU, contiguous, 16 B aligned, R and C multiples of
// 16 (what the FP8 GEMM itself requires of every operand)
inline void fp8_check_input(const torch::Tensor& x) {
  CHECK_BF16_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, "fp8 quantisation expects a 2-D [R, C] tensor");
  TORCH_CHECK(x.size(0) > 0 && x.size(1) > 0 && x.size(0) % 16 == 0 &&
                  x.size(1) % 16 == 0,
              "fp8 quantisation requires R and C to be positive multiples "
              "of 16, got [", x.size(0), ", ", x.size(1), "]");
  TORCH_CHECK(x.size(0) <= INT32_MAX && x.size(1) <= INT32_MAX,
              "fp8 quantisation: R and C must fit in int32");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "fp8 quantisation requires a 16-byte aligned tensor");
}

// f32 [2] on x's device: {448 / max(amax, 1e-12), max(amax, 1e-12) / 448}
torch::Tensor fp8_amax_scale(torch::Tensor x) {
  fp8_check_input(x);
  auto partials = torch::empty({(int64_t)fp8_amax_blocks(x.numel())},
                               x.options().dtype(torch::kInt));
  auto scales = torch::empty({2}, x.options().dtype(torch::kFloat));
  fp8_amax_scale_launch(x.data_ptr(), x.numel(), partials.data_ptr(),
                        scales.data_ptr<float>(), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return scales;
}

// (q [R, C], qt [C, R]) in e4m3; an output not asked for comes back None
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
fp8_cast_transpose(torch::Tensor x, torch::Tensor scale, bool rowwise,
                   bool transposed) {
  fp8_check_input(x);
  TORCH_CHECK(rowwise || transposed,
              "fp8_cast_transpose: ask for at least one output");
  TORCH_CHECK(scale.is_cuda() && scale.device() == x.device(),
              "scale must be on x's device");
  TORCH_CHECK(scale.dtype() == torch::kFloat && scale.numel() == 1,
              "scale must be a single f32 value");
  const int64_t R = x.size(0), C = x.size(1);
  auto opts = x.options().dtype(at::kFloat8_e4m3fn);
  c10::optional<torch::Tensor> q, qt;
  if (rowwise) q = torch::empty({R, C}, opts);
  if (transposed) qt = torch::empty({C, R}, opts);
  fp8_cast_transpose_launch(x.data_ptr(), scale.data_ptr<float>(),
                            q ? q->data_ptr() : nullptr,
                            qt ? qt->data_ptr() : nullptr, (int)R, (int)C,
                            cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {q, qt};
}

// ---------------- fp8 delayed scaling (fp8_delayed.hip) ----------------
inline void fp8_check_scale(const torch::Tensor& scale,
                            const torch::Tensor& x) {
  TORCH_CHECK(scale.is_cuda() && scale.device() == x.device(),
              "scale must be on the input's device");
  TORCH_CHECK(scale.dtype() == torch::kFloat && scale.numel() == 1,
              "scale must be a single f32 value");
}

inline torch::Tensor fp8_new_partials(const torch::Tensor& x, int64_t R,
                                      int64_t C) {
  const int64_t tiles = fp8_tiles((int)R, (int)C);
  TORCH_CHECK(tiles <= INT32_MAX, "fp8 quantisation: too many tiles");
  return torch::empty({tiles}, x.options().dtype(torch::kInt));
}

// fp8_cast_transpose with the scale given, plus the per-tile amax partials
// (int32: sign-cleared bf16 bit patterns) for fp8_history_update
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>,
           torch::Tensor>
fp8_cast_amax(torch::Tensor x, torch::Tensor scale, bool rowwise,
              bool transposed) {
  fp8_check_input(x);
  TORCH_CHECK(rowwise || transposed,
              "fp8_cast_amax: ask for at least one output");
  fp8_check_scale(scale, x);
  const int64_t R = x.size(0), C = x.size(1);
  auto opts = x.options().dtype(at::kFloat8_e4m3fn);
  c10::optional<torch::Tensor> q, qt;
  if (rowwise) q = torch::empty({R, C}, opts);
  if (transposed) qt = torch::empty({C, R}, opts);
  auto partials = fp8_new_partials(x, R, C);
  fp8_cast_amax_launch(x.data_ptr(), scale.data_ptr<float>(),
                       q ? q->data_ptr() : nullptr,
                       qt ? qt->data_ptr() : nullptr, partials.data_ptr(),
                       (int)R, (int)C, cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {q, qt, partials};
}

// gate_up [R, 2I] bf16 -> (hq [R, I], hqt [I, R], partials) of
// h = silu(gate) * up, which is never written
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> silu_mul_fp8(
    torch::Tensor gu, torch::Tensor scale) {
  CHECK_BF16_CONTIG(gu);
  TORCH_CHECK(gu.dim() == 2, "silu_mul_fp8 expects gate_up as [R, 2I]");
  const int64_t R = gu.size(0), I = gu.size(1) / 2;
  TORCH_CHECK(R > 0 && I > 0 && R % 16 == 0 && gu.size(1) % 32 == 0,
              "silu_mul_fp8 requires R and I to be positive multiples of "
              "16, got [", R, ", 2 * ", I, "]");
  TORCH_CHECK(R <= INT32_MAX && gu.size(1) <= INT32_MAX,
              "silu_mul_fp8: R and 2I must fit in int32");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(gu.data_ptr()) % 16 == 0,
              "silu_mul_fp8 requires a 16-byte aligned tensor");
  fp8_check_scale(scale, gu);
  auto opts = gu.options().dtype(at::kFloat8_e4m3fn);
  auto q = torch::empty({R, I}, opts);
  auto qt = torch::empty({I, R}, opts);
  auto partials = fp8_new_partials(gu, R, I);
  silu_mul_fp8_launch(gu.data_ptr(), scale.data_ptr<float>(), q.data_ptr(),
                      qt.data_ptr(), partials.data_ptr(), (int)R, (int)I,
                      cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {q, qt, partials};
}

// Fold the partials into this step's amax, put it into history[slot] in
// place (slot < 0: into every slot) and return a fresh f32 [2] = {scale,
// inv_scale} of max(history)
torch::Tensor fp8_history_update(torch::Tensor partials,
                                 torch::Tensor history, int64_t slot) {
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.dtype() == torch::kInt && partials.numel() > 0 &&
                  partials.numel() <= INT32_MAX,
              "partials must be a non-empty contiguous int32 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(partials.data_ptr()) % 16 == 0,
              "partials must be 16-byte aligned");
  TORCH_CHECK(history.is_cuda() && history.device() == partials.device() &&
                  history.is_contiguous() &&
                  history.dtype() == torch::kFloat && history.dim() == 1 &&
                  history.numel() > 0 && history.numel() <= 1024,
              "history must be a contiguous f32 [L] tensor, 1 <= L <= 1024, "
              "on the partials' device");
  TORCH_CHECK(slot < history.numel(), "slot ", slot,
              " is outside the history of ", history.numel());
  auto out = torch::empty({2}, history.options());
  fp8_history_update_launch(partials.data_ptr(), (int)partials.numel(),
                            history.data_ptr<float>(), (int)history.numel(),
                            (int)(slot < 0 ? -1 : slot),
                            out.data_ptr<float>(), cur_stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// ---------------- attention ----------------
// doc_start / doc_end are the [B,S] int32 tables of ops/doc_mask.py (their
// contents are the caller's contract; the kernels only keep a bad table
// from moving loads out of bounds); an undefined tensor = plain causal
#define CHECK_DOC_TABLE(t, q)                                              \
  TORCH_CHECK((t).is_cuda() && (t).device() == (q).device(),               \
              #t " must be on q's device");                                \
  TORCH_CHECK((t).dtype() == torch::kInt, #t " must be int32");            \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");              \
  TORCH_CHECK((t).dim() == 2 && (t).size(0) == (q).size(0) &&              \
              (t).size(1) == (q).size(1), #t " must be [B,S]")

struct AttnDims {
  int B, S, Hq, Hkv, D;
};

// the checks every attention entry point makes of q / k / v
AttnDims attn_check_qkv(const torch::Tensor& q, const torch::Tensor& k,
                        const torch::Tensor& v) {
  CHECK_BF16_CONTIG(q);
  CHECK_BF16_CONTIG(k);
  CHECK_BF16_CONTIG(v);
  TORCH_CHECK(q.dim() == 4, "q must be [B,S,Hq,D]");
  TORCH_CHECK(k.dim() == 4 && k.size(0) == q.size(0) &&
                  k.size(1) == q.size(1) && k.size(3) == q.size(3),
              "k must be [B,S,Hkv,D]");
  TORCH_CHECK(v.sizes() == k.sizes(), "v must be [B,S,Hkv,D]");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
              "k and v must be on q's device");
  const AttnDims d = {(int)q.size(0), (int)q.size(1), (int)q.size(2),
                      (int)k.size(2), (int)q.size(3)};
  TORCH_CHECK(d.Hq % d.Hkv == 0, "GQA requires Hq % Hkv == 0");
  TORCH_CHECK(d.D == 64 || d.D == 128, "head dim must be 64 or 128");
  return d;
}

std::vector<torch::Tensor> attn_fwd_impl(const torch::Tensor& q,
                                         const torch::Tensor& k,
                                         const torch::Tensor& v,
                                         const torch::Tensor& doc_start,
                                         double scale) {
  const AttnDims d = attn_check_qkv(q, k, v);
  const bool doc = doc_start.defined();
  if (doc) {
    CHECK_DOC_TABLE(doc_start, q);
  }
  auto o = torch::empty_like(q);
  auto lse = torch::empty({(int64_t)d.B, (int64_t)d.Hq, (int64_t)d.S},
                          q.options().dtype(torch::kFloat));
  attn_fwd_launch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                  lse.data_ptr<float>(),
                  doc ? doc_start.data_ptr<int>() : nullptr, d.B, d.S, d.Hq,
                  d.Hkv, d.D, (float)scale, cur_stream());
  return {o, lse};
}

std::vector<torch::Tensor> attn_bwd_impl(
    const torch::Tensor& dout, const torch::Tensor& q, const torch::Tensor& k,
    const torch::Tensor& v, const torch::Tensor& o, const torch::Tensor& lse,
    const torch::Tensor& doc_start, const torch::Tensor& doc_end,
    double scale) {
  const AttnDims d = attn_check_qkv(q, k, v);
  CHECK_BF16_CONTIG(dout);
  CHECK_BF16_CONTIG(o);
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes(),
              "dout and o must be [B,S,Hq,D] like q");
  TORCH_CHECK(lse.is_cuda() && lse.dtype() == torch::kFloat &&
                  lse.is_contiguous() && lse.dim() == 3 &&
                  lse.size(0) == d.B && lse.size(1) == d.Hq &&
                  lse.size(2) == d.S,
              "lse must be a contiguous cuda f32 [B,Hq,S]");
  TORCH_CHECK(dout.device() == q.device() && o.device() == q.device() &&
                  lse.device() == q.device(),
              "dout, o and lse must be on q's device");
  const bool doc = doc_start.defined();
  if (doc) {
    CHECK_DOC_TABLE(doc_start, q);
    CHECK_DOC_TABLE(doc_end, q);
  }
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  auto delta = torch::empty({(int64_t)d.B, (int64_t)d.Hq, (int64_t)d.S},
                            q.options().dtype(torch::kFloat));
  attn_bwd_launch(dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                  o.data_ptr(), lse.data_ptr<float>(),
                  delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                  dv.data_ptr(), doc ? doc_start.data_ptr<int>() : nullptr,
                  doc ? doc_end.data_ptr<int>() : nullptr, d.B, d.S, d.Hq,
                  d.Hkv, d.D, (float)scale, cur_stream());
  return {dq, dk, dv};
}

// the Python-visible names: one pair per mode
std::vector<torch::Tensor> attn_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, double scale) {
  return attn_fwd_impl(q, k, v, torch::Tensor(), scale);
}
std::vector<torch::Tensor> attn_fwd_doc(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor v,
                                        torch::Tensor doc_start,
                                        double scale) {
  return attn_fwd_impl(q, k, v, doc_start, scale);
}
std::vector<torch::Tensor> attn_bwd(torch::Tensor dout, torch::Tensor q,
                                    torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse,
                                    double scale) {
  return attn_bwd_impl(dout, q, k, v, o, lse, torch::Tensor(), torch::Tensor(),
                       scale);
}
std::vector<torch::Tensor> attn_bwd_doc(torch::Tensor dout, torch::Tensor q,
                                        torch::Tensor k, torch::Tensor v,
                                        torch::Tensor o, torch::Tensor lse,
                                        torch::Tensor doc_start,
                                        torch::Tensor doc_end, double scale) {
  return attn_bwd_impl(dout, q, k, v, o, lse, doc_start, doc_end, scale);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("rope", &rope);
  m.def("add_rmsnorm_fwd", &add_rmsnorm_fwd);
  m.def("add_rmsnorm_bwd", &add_rmsnorm_bwd);
  m.def("qkv_rope_fwd", &qkv_rope_fwd);
  m.def("qkv_rope_bwd", &qkv_rope_bwd);
  m.def("qkv_norm_rope_fwd", &qkv_norm_rope_fwd);
  m.def("qkv_norm_rope_bwd", &qkv_norm_rope_bwd);
  m.def("moe_router_fwd", &moe_router_fwd);
  m.def("moe_router_bwd", &moe_router_bwd);
  m.def("moe_router_aux_fwd", &moe_router_aux_fwd);
  m.def("moe_router_aux_bwd", &moe_router_aux_bwd);
  m.def("moe_dispatch_index", &moe_dispatch_index);
  m.def("moe_scatter", &moe_scatter);
  m.def("moe_combine", &moe_combine);
  m.def("moe_combine_bwd", &moe_combine_bwd);
  m.def("moe_gemm_rows", &moe_gemm_rows);
  m.def("moe_gemm_dw", &moe_gemm_dw);
  m.def("moe_row_src", &moe_row_src);
  m.def("moe_gemm_rows_gather", &moe_gemm_rows_gather);
  m.def("moe_gemm_dw_gather", &moe_gemm_dw_gather);
  m.def("moe_row_w", &moe_row_w);
  m.def("moe_gemm_gu_swiglu", &moe_gemm_gu_swiglu);
  m.def("moe_gemm_da_swiglu", &moe_gemm_da_swiglu);
  m.def("silu_mul_fwd", &silu_mul_fwd);
  m.def("silu_mul_bwd", &silu_mul_bwd);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
  m.def("embedding_bwd_sorted", &embedding_bwd_sorted);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_fwd_sharded", &ce_fwd_sharded);
  m.def("ce_bwd", &ce_bwd, py::arg("logits"), py::arg("labels"),
        py::arg("lse"), py::arg("scale"), py::arg("S_out"),
        py::arg("vocab_start"), py::arg("ignore_index"),
        py::arg("sharded"), py::arg("scale_t") = c10::nullopt);
  m.def("adamw_step", &adamw_step);
  m.def("adamw_step_clipped", &adamw_step_clipped);
  m.def("adamw_master_step", &adamw_master_step);
  m.def("grad_sqsum", &grad_sqsum);
  m.def("grad_scale_", &grad_scale_);
  m.def("fp8_amax_scale", &fp8_amax_scale);
  m.def("fp8_cast_transpose", &fp8_cast_transpose);
  m.def("fp8_cast_amax", &fp8_cast_amax);
  m.def("silu_mul_fp8", &silu_mul_fp8);
  m.def("fp8_history_update", &fp8_history_update);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_fwd_doc", &attn_fwd_doc);
  m.def("attn_bwd_doc", &attn_bwd_doc);
}
