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
  m.def("silu_mul_fwd", &silu_mul_fwd);
  m.def("silu_mul_bwd", &silu_mul_bwd);
  m.def("embedding_fwd", &embedding_fwd);
  m.def("embedding_bwd", &embedding_bwd);
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
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_fwd_doc", &attn_fwd_doc);
  m.def("attn_bwd_doc", &attn_bwd_doc);
}
