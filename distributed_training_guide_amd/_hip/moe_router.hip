// Fused mixture-of-experts router for gfx950: softmax -> top-k ->
// renormalise over the router GEMM's bf16 logits [T, E] in one pass, and its
// backward in one pass (ops/moe.py).
//
// Forward outputs: topk_idx int32 [T, k] and topk_w f32 [T, k].  Selection
// runs on the raw logits widened to f32 (exact), descending, a tie going to
// the lower expert index: the first k of a stable descending sort.  With
// NORM (Qwen3-MoE's norm_topk_prob) the weights are the softmax over the k
// selected logits, otherwise the full softmax's values at the selection.
// Either way w_j = exp(x_j - m) / Z with m the row maximum, which is the
// first selected value, and Z summed over the selection (NORM) or the row.
// Backward: with p_e = exp(x_e - m) / Z (zero outside the selection under
// NORM) and g_e the incoming d_topk_w of a selected expert (zero otherwise),
//   dlogits_e = p_e * (g_e - sum_e' p_e' g_e')
// rounded once to bf16.  Nothing but the logits and topk_idx is kept from
// the forward: p is recomputed.
//
// Mapping.  A token's E logits live in the lanes of one wave: LPT = min(E, 64)
// lanes hold VPL = E / LPT values each (2 adjacent experts, one 4-byte load,
// at E = 128), and 64 / LPT tokens share a wave.  LPT divides 64, so a
// token's lane group never straddles a wavefront and every reduction is a
// __shfl_xor butterfly over log2(LPT) steps.  Top-k is k rounds of a
// butterfly arg-max over (value, index): every lane of the group ends the
// round with the same winner, the lane that owns it retires it, and the
// group's lane j keeps round j's winner for the store.  No LDS, no second
// pass, no register array with a run-time index; token and expert come from
// block, wave and lane with shifts and masks only.
#include "common.h"
#include "launchers.h"
#include "moe_router_common.h"

template <int E, bool NORM>
__global__ void __launch_bounds__(256) moe_router_fwd_kernel(
    const short* __restrict__ logits, int* __restrict__ topk_idx,
    float* __restrict__ topk_w, int64_t T, int k) {
  constexpr int LPT = E < WAVE ? E : WAVE;
  constexpr int VPL = E / LPT;
  constexpr int TPW = WAVE / LPT;
  constexpr int RETIRED = 2 * E;  // index of a retired value: loses every tie
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int sl = lane & (LPT - 1);  // lane within the token's group
  const int e0 = sl * VPL;
  const int64_t step = (int64_t)gridDim.x * MR_WAVES * TPW;
  const int64_t first = ((int64_t)blockIdx.x * MR_WAVES + wid) * TPW;
  // the bound is on the wave's first token: all lanes of a wave leave together
  for (int64_t t0 = first; t0 < T; t0 += step) {
    const int64_t t = t0 + (TPW > 1 ? lane / LPT : 0);
    const bool live = t < T;
    float x0 = 0.f, x1 = -INFINITY;
    if (live) mr_load<E, VPL>(logits, t, e0, x0, x1);

    bool took0 = false, took1 = (VPL == 1);
    float m = 0.f, z = 0.f;  // row max (round 0's winner), sum of exp
    float myv = 0.f;
    int myi = 0;
    for (int j = 0; j < k; ++j) {
      // the lane's best value still in play; a retired slot stands as
      // (-inf, RETIRED) and so loses to a live -inf logit as well
      float bv = took0 ? -INFINITY : x0;
      int bi = took0 ? RETIRED : e0;
      if constexpr (VPL == 2) {
        const float cv = took1 ? -INFINITY : x1;
        const int ci = took1 ? RETIRED : e0 + 1;
        if (mr_better(cv, ci, bv, bi)) {
          bv = cv;
          bi = ci;
        }
      }
#pragma unroll
      for (int off = LPT / 2; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, WAVE);
        const int oi = __shfl_xor(bi, off, WAVE);
        if (mr_better(ov, oi, bv, bi)) {
          bv = ov;
          bi = oi;
        }
      }
      took0 = took0 || bi == e0;
      if constexpr (VPL == 2) took1 = took1 || bi == e0 + 1;
      if (j == 0) m = bv;
      if (NORM) z += expf(bv - m);
      if (sl == j) {
        myv = bv;
        myi = bi;
      }
    }
    if (!NORM) {
      float zz = expf(x0 - m);
      if constexpr (VPL == 2) zz += expf(x1 - m);
      z = group_sum<LPT>(zz);
    }
    if (live && sl < k) {
      topk_idx[t * k + sl] = myi;
      topk_w[t * k + sl] = expf(myv - m) / z;
    }
  }
}

template <int E, bool NORM>
__global__ void __launch_bounds__(256) moe_router_bwd_kernel(
    const short* __restrict__ logits, const int* __restrict__ topk_idx,
    const float* __restrict__ d_topk_w, short* __restrict__ dlogits,
    int64_t T, int k) {
  constexpr int LPT = E < WAVE ? E : WAVE;
  constexpr int VPL = E / LPT;
  constexpr int TPW = WAVE / LPT;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int sl = lane & (LPT - 1);
  const int e0 = sl * VPL;
  const int64_t step = (int64_t)gridDim.x * MR_WAVES * TPW;
  const int64_t first = ((int64_t)blockIdx.x * MR_WAVES + wid) * TPW;
  for (int64_t t0 = first; t0 < T; t0 += step) {
    const int64_t t = t0 + (TPW > 1 ? lane / LPT : 0);
    const bool live = t < T;
    float x0 = 0.f, x1 = -INFINITY;
    if (live) mr_load<E, VPL>(logits, t, e0, x0, x1);
    // the selection and its incoming gradient: k broadcast loads per group
    bool sel0 = false, sel1 = false;
    float g0 = 0.f, g1 = 0.f;
    if (live) {
      for (int j = 0; j < k; ++j) {
        const int e = topk_idx[t * k + j];
        const float g = d_topk_w[t * k + j];
        if (e == e0) {
          sel0 = true;
          g0 = g;
        }
        if (VPL == 2 && e == e0 + 1) {
          sel1 = true;
          g1 = g;
        }
      }
    }
    float mx = x0;
    if constexpr (VPL == 2) mx = fmaxf(x0, x1);
    const float m = group_max<LPT>(mx);
    float p0 = (NORM && !sel0) ? 0.f : expf(x0 - m);
    float p1 = (VPL == 1 || (NORM && !sel1)) ? 0.f : expf(x1 - m);
    const float rz = 1.0f / group_sum<LPT>(p0 + p1);
    p0 *= rz;
    p1 *= rz;
    const float dot = group_sum<LPT>(p0 * g0 + p1 * g1);
    if (!live) continue;
    const short d0 = f2bf(p0 * (g0 - dot));
    if constexpr (VPL == 2) {
      const short d1 = f2bf(p1 * (g1 - dot));
      *reinterpret_cast<uint32_t*>(dlogits + t * E + e0) =
          (uint32_t)(uint16_t)d0 | ((uint32_t)(uint16_t)d1 << 16);
    } else {
      dlogits[t * E + e0] = d0;
    }
  }
}

extern "C" {
void moe_router_fwd_launch(const void* logits, int* topk_idx, float* topk_w,
                           int64_t T, int E, int k, int norm, hipStream_t s) {
  if (T < 1) return;
  MR_DISPATCH(moe_router_fwd_kernel, dim3(mr_grid(T, E, MR_GRID_CAP)),
              (const short*)logits, topk_idx, topk_w, T, k);
}

void moe_router_bwd_launch(const void* logits, const int* topk_idx,
                           const float* d_topk_w, void* dlogits, int64_t T,
                           int E, int k, int norm, hipStream_t s) {
  if (T < 1) return;
  MR_DISPATCH(moe_router_bwd_kernel, dim3(mr_grid(T, E, MR_GRID_CAP)),
              (const short*)logits, topk_idx, d_topk_w, (short*)dlogits, T,
              k);
}
}
