// The router of moe_router.hip with the two standard router regularisers
// produced by the same kernels (ops/moe.py, moe_router(..., aux=True)): the
// load-balancing loss of Switch / HF and the router z-loss of ST-MoE, over
// the T tokens of one layer, with their gradients.
//
// With p[t, e] the FULL softmax of a logits row (in both modes: NORM only
// changes the routing weights), c[e] the number of the T*k slots routed to
// expert e and lse[t] = log sum_e exp(x[t, e]):
//   P[e] = (1/T) sum_t p[t, e]
//   aux  = E * sum_e (c[e] / T) * P[e]      (= k under uniform routing)
//   z    = (1/T) sum_t lse[t]^2
// c carries no gradient.  With the upstream scalars g_aux and g_z and
// a[e] = g_aux * E * c[e] / T^2 the backward adds two terms to the routing
// term of moe_router_bwd_kernel:
//   dlogits[t, e] = pr_e * (g_e - sum pr g)
//                 + p_e * (a_e - sum_e' p_e' a_e')
//                 + g_z * (2/T) * lse_t * p_e
// summed in f32 and rounded to bf16 once.  pr is the routing probability
// (p itself without NORM, the softmax over the selection with it).
//
// Forward.  The mapping, the top-k rounds and the arithmetic of the routing
// outputs are moe_router_fwd_kernel's, so topk_idx and topk_w are its bits.
// Round 0's winner is the row maximum m, so the full softmax costs one more
// exp per value and one butterfly for the row's Z (NORM; without NORM that
// sum is the one the routing weights need anyway).  A lane owns the same one
// or two experts for every token it sees, so it accumulates over its
// grid-stride token loop, in registers: the probability of its experts, the
// number of tokens that took them (it knows: it retired them), and on the
// group's lane 0 lse^2.  Only live tokens contribute: the tail groups of a
// ragged last wave add nothing.  After the loop the block folds once, in a
// fixed order: the 64/E lane groups of a wave that own the same experts by
// __shfl_xor over the group index, the four waves through LDS, and one row of
// 2E + 1 partials [P*T | c | sum lse^2] goes out by ordinary stores.  The
// count columns are int32 bit patterns in the f32 row, so they stay exact.
// The grid is capped at MRA_GRID_CAP blocks so that the second kernel's fold
// stays short.
//
// Finish.  One block folds the [nblocks, 2E + 1] rows in double, column by
// column in a fixed order, and writes counts[E] (exact) and the two scalars.
// The grad_norm.hip pattern: no atomics, no pre-zeroed buffer, no host sync,
// bitwise reproducible.
//
// Backward.  p and lse are recomputed from the saved logits; under NORM the
// selection-normalised pr and the full-row p come from one set of exp
// values.  a[e] of the lane's experts is formed once before the token loop
// from counts and the device scalars g_aux and g_z, which the host never
// reads.  It keeps no accumulator, so it takes the plain router's grid.
#include "common.h"
#include "launchers.h"
#include "moe_router_common.h"

// two blocks per CU of the 256: enough waves to hide the butterflies' latency
// while the finishing block reads at most 512 rows
constexpr int MRA_GRID_CAP = 512;
constexpr int MRA_FINISH_THREADS = 1024;
constexpr int MRA_MAX_COLS = 2 * 128 + 1;

template <int E, bool NORM>
__global__ void __launch_bounds__(256) moe_router_aux_fwd_kernel(
    const short* __restrict__ logits, int* __restrict__ topk_idx,
    float* __restrict__ topk_w, float* __restrict__ partials, int64_t T,
    int k) {
  constexpr int LPT = E < WAVE ? E : WAVE;
  constexpr int VPL = E / LPT;
  constexpr int TPW = WAVE / LPT;
  constexpr int RETIRED = 2 * E;
  constexpr int NCOL = 2 * E + 1;
  __shared__ float sh[MR_WAVES][NCOL];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int sl = lane & (LPT - 1);
  const int e0 = sl * VPL;
  const int64_t step = (int64_t)gridDim.x * MR_WAVES * TPW;
  const int64_t first = ((int64_t)blockIdx.x * MR_WAVES + wid) * TPW;
  float acc_p0 = 0.f, acc_p1 = 0.f, acc_z = 0.f;
  int acc_c0 = 0, acc_c1 = 0;
  for (int64_t t0 = first; t0 < T; t0 += step) {
    const int64_t t = t0 + (TPW > 1 ? lane / LPT : 0);
    const bool live = t < T;
    float x0 = 0.f, x1 = -INFINITY;
    if (live) mr_load<E, VPL>(logits, t, e0, x0, x1);

    bool took0 = false, took1 = (VPL == 1);
    float m = 0.f, z = 0.f;
    float myv = 0.f;
    int myi = 0;
    for (int j = 0; j < k; ++j) {
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
    // the full row's exp values and their sum, in both modes
    const float ex0 = expf(x0 - m);
    float ex1 = 0.f;
    float zz = ex0;
    if constexpr (VPL == 2) {
      ex1 = expf(x1 - m);
      zz += ex1;
    }
    const float zf = group_sum<LPT>(zz);
    if (!NORM) z = zf;
    if (live && sl < k) {
      topk_idx[t * k + sl] = myi;
      topk_w[t * k + sl] = expf(myv - m) / z;
    }
    if (live) {
      const float rzf = 1.0f / zf;
      acc_p0 += ex0 * rzf;
      acc_c0 += took0 ? 1 : 0;
      if constexpr (VPL == 2) {
        acc_p1 += ex1 * rzf;
        acc_c1 += took1 ? 1 : 0;
      }
      if (sl == 0) {
        const float lse = m + logf(zf);
        acc_z += lse * lse;
      }
    }
  }
  // (1) the lane groups of a wave own the same experts
#pragma unroll
  for (int off = LPT; off < WAVE; off <<= 1) {
    acc_p0 += __shfl_xor(acc_p0, off, WAVE);
    acc_c0 += __shfl_xor(acc_c0, off, WAVE);
    acc_z += __shfl_xor(acc_z, off, WAVE);
  }
  // (2) the four waves, through LDS
  if (lane < LPT) {
    sh[wid][e0] = acc_p0;
    sh[wid][E + e0] = __int_as_float(acc_c0);
    if constexpr (VPL == 2) {
      sh[wid][e0 + 1] = acc_p1;
      sh[wid][E + e0 + 1] = __int_as_float(acc_c1);
    }
    if (lane == 0) sh[wid][2 * E] = acc_z;
  }
  __syncthreads();
  // (3) one row per block
  float* row = partials + (int64_t)blockIdx.x * NCOL;
  for (int c = threadIdx.x; c < NCOL; c += 256) {
    if (c >= E && c < 2 * E) {
      const int n = (__float_as_int(sh[0][c]) + __float_as_int(sh[1][c])) +
                    (__float_as_int(sh[2][c]) + __float_as_int(sh[3][c]));
      row[c] = __int_as_float(n);
    } else {
      row[c] = (sh[0][c] + sh[1][c]) + (sh[2][c] + sh[3][c]);
    }
  }
}

// <<<1, 1024>>>: fold partials [nblocks, 2E + 1].  Thread (g, c) sums the
// rows g, g + rg, ... of column c in double, thread c then the rg row groups
// in order; thread 0 forms the scalars.
__global__ void __launch_bounds__(MRA_FINISH_THREADS)
moe_router_aux_finish_kernel(const float* __restrict__ partials, int nblocks,
                             int E, int64_t T, int* __restrict__ counts,
                             float* __restrict__ aux, float* __restrict__ z) {
  __shared__ double sh[MRA_FINISH_THREADS];
  __shared__ double tot[MRA_MAX_COLS];
  const int ncol = 2 * E + 1;
  const int rg = MRA_FINISH_THREADS / ncol;  // 3 at E = 128, 60 at E = 8
  const int g = threadIdx.x / ncol;
  const int c = threadIdx.x - g * ncol;
  const bool is_count = c >= E && c < 2 * E;
  double acc = 0.0;
  if (g < rg) {
#pragma unroll 4
    for (int r = g; r < nblocks; r += rg) {
      const float v = partials[(int64_t)r * ncol + c];
      acc += is_count ? (double)__float_as_int(v) : (double)v;
    }
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (g == 0) {
    double t = 0.0;
    for (int j = 0; j < rg; ++j) t += sh[j * ncol + c];
    tot[c] = t;
    if (is_count) counts[c - E] = (int)t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int e = 0; e < E; ++e) s += tot[E + e] * tot[e];
    const double Td = (double)T;
    *aux = (float)(s * (double)E / (Td * Td));
    *z = (float)(tot[2 * E] / Td);
  }
}

template <int E, bool NORM>
__global__ void __launch_bounds__(256) moe_router_aux_bwd_kernel(
    const short* __restrict__ logits, const int* __restrict__ topk_idx,
    const float* __restrict__ d_topk_w, const int* __restrict__ counts,
    const float* __restrict__ g_aux, const float* __restrict__ g_z,
    short* __restrict__ dlogits, int64_t T, int k) {
  constexpr int LPT = E < WAVE ? E : WAVE;
  constexpr int VPL = E / LPT;
  constexpr int TPW = WAVE / LPT;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int sl = lane & (LPT - 1);
  const int e0 = sl * VPL;
  const int64_t step = (int64_t)gridDim.x * MR_WAVES * TPW;
  const int64_t first = ((int64_t)blockIdx.x * MR_WAVES + wid) * TPW;
  // a[e] of the lane's experts and the z term's factor, once
  const float Tf = (float)T;
  const float ascale = *g_aux * (float)E / (Tf * Tf);
  const float a0 = ascale * (float)counts[e0];
  float a1 = 0.f;
  if constexpr (VPL == 2) a1 = ascale * (float)counts[e0 + 1];
  const float zc = *g_z * 2.0f / Tf;
  for (int64_t t0 = first; t0 < T; t0 += step) {
    const int64_t t = t0 + (TPW > 1 ? lane / LPT : 0);
    const bool live = t < T;
    float x0 = 0.f, x1 = -INFINITY;
    if (live) mr_load<E, VPL>(logits, t, e0, x0, x1);
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
    // one set of exp values serves the full row and the selection
    const float ex0 = expf(x0 - m);
    const float ex1 = VPL == 1 ? 0.f : expf(x1 - m);
    const float zf = group_sum<LPT>(ex0 + ex1);
    const float rzf = 1.0f / zf;
    const float p0 = ex0 * rzf, p1 = ex1 * rzf;
    float pr0 = p0, pr1 = p1;
    if constexpr (NORM) {
      const float s0 = sel0 ? ex0 : 0.f, s1 = sel1 ? ex1 : 0.f;
      const float rzr = 1.0f / group_sum<LPT>(s0 + s1);
      pr0 = s0 * rzr;
      pr1 = s1 * rzr;
    }
    const float dot = group_sum<LPT>(pr0 * g0 + pr1 * g1);
    const float dota = group_sum<LPT>(p0 * a0 + p1 * a1);
    if (!live) continue;
    const float zt = zc * (m + logf(zf));
    const short d0 = f2bf(pr0 * (g0 - dot) + p0 * (a0 - dota) + zt * p0);
    if constexpr (VPL == 2) {
      const short d1 = f2bf(pr1 * (g1 - dot) + p1 * (a1 - dota) + zt * p1);
      *reinterpret_cast<uint32_t*>(dlogits + t * E + e0) =
          (uint32_t)(uint16_t)d0 | ((uint32_t)(uint16_t)d1 << 16);
    } else {
      dlogits[t * E + e0] = d0;
    }
  }
}

extern "C" {
int moe_router_aux_grid(int64_t T, int E) {
  return mr_grid(T, E, MRA_GRID_CAP);
}

void moe_router_aux_fwd_launch(const void* logits, int* topk_idx,
                               float* topk_w, float* partials, int* counts,
                               float* aux, float* z, int64_t T, int E, int k,
                               int norm, hipStream_t s) {
  if (T < 1) return;
  const int nblocks = moe_router_aux_grid(T, E);
  MR_DISPATCH(moe_router_aux_fwd_kernel, dim3(nblocks), (const short*)logits,
              topk_idx, topk_w, partials, T, k);
  hipLaunchKernelGGL(moe_router_aux_finish_kernel, dim3(1),
                     dim3(MRA_FINISH_THREADS), 0, s, (const float*)partials,
                     nblocks, E, T, counts, aux, z);
}

void moe_router_aux_bwd_launch(const void* logits, const int* topk_idx,
                               const float* d_topk_w, const int* counts,
                               const float* g_aux, const float* g_z,
                               void* dlogits, int64_t T, int E, int k,
                               int norm, hipStream_t s) {
  if (T < 1) return;
  MR_DISPATCH(moe_router_aux_bwd_kernel, dim3(mr_grid(T, E, MR_GRID_CAP)),
              (const short*)logits, topk_idx, d_topk_w, counts, g_aux, g_z,
              (short*)dlogits, T, k);
}
}
