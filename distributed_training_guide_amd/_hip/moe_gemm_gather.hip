// Gather-fused expert GEMMs for gfx950: the forward and the weight gradient
// of the gate_up projection read the tokens through a row index, so the
// expert-sorted copy xp[dest[t*k + j]] = x[t] of moe_scatter never exists.
//
//   x [T, K] bf16, tokens in their own order; row_src int32 [N], N = T*k:
//   the token of every row of the expert-sorted layout, row_src[dest[s]] =
//   s / k (moe_row_src_kernel); weight [E, M, K]; offs int32 [E].
//
//   forward  y[r, :] = x[row_src[r], :] . weight[e]^T  moe_gemm_rows_gather_kernel
//   dW       dw[e]   = dy[rows e]^T . x[row_src[rows e]]  moe_gemm_dw_gather_kernel
//
// Tiling, work search, double buffering, MFMA step and epilogue are those of
// moe_gemm.hip (moe_gemm_tile.h); the arithmetic and its order are the same,
// so the results are the bits moe_gemm.hip gives on the scattered copy.  What
// differs is where the 64 x 64 images of the token operand come from.
// global_load_lds takes its global address per lane and only its LDS base
// must be wave-uniform, so a lane can fetch its 16 bytes of an image row from
// any row of x: the LDS side stays image + (wid*2 + j)*512, the global side
// becomes x + row_src[row]*K + column.
//
// Forward.  In stage_img's mapping a lane stages the same rows of the tile at
// every K-step: rows j*32 + lane/2 (j = 0, 1) of both 64-row images.  Each
// lane therefore loads its four source indices once, after the tile search,
// turns them into element offsets and keeps those across the K loop, where a
// step only adds its column.
//
// dW.  The contraction runs over the group's rows, 64 a step, so a lane's
// two indices change every step.  The staging of step s+1 is issued during
// step s; were its indices loaded there too, every stage would wait on a
// dependent load.  The index loads run one step further ahead: step s issues
// the DMA of step s+1 from indices that arrived during step s-1 and loads
// the indices of step s+2.  The barrier that ends a step waits for the DMA
// anyway, and the index load, issued before it, has landed by then.
//
// Every index is clamped into [0, T), as offs is clamped into [0, N]: a
// table outside the contract gives wrong numbers, never an access out of
// bounds.
#include "moe_gemm_tile.h"
#include "launchers.h"

constexpr int RS_MAX_K = 8;

// row_src[dest[t*k + j]] = t.  One thread per token walks its k slots (no
// integer divide); dest is a permutation of [0, T*k), so every element is
// written exactly once: no atomics, nothing cleared first.  A value outside
// [0, T*k) is dropped.
__global__ void __launch_bounds__(256) moe_row_src_kernel(
    const int* __restrict__ dest, int* __restrict__ row_src, int T, int k) {
  const int N = T * k;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += gridDim.x * 256) {
    const int* d = dest + (int64_t)t * k;
    int r[RS_MAX_K];  // all loads first; slots past k re-read the last one
#pragma unroll
    for (int j = 0; j < RS_MAX_K; ++j) r[j] = d[min(j, k - 1)];
#pragma unroll
    for (int j = 0; j < RS_MAX_K; ++j)
      if (j < k && (unsigned)r[j] < (unsigned)N) row_src[r[j]] = t;
  }
}

// out[r, :] = x[row_src[r], :] . weight[e]^T for the rows r of group e:
// x [T, L], weight [E, C, L], out [N, C].  Grid as moe_gemm_rows_kernel.
__global__ void __launch_bounds__(256, 2) moe_gemm_rows_gather_kernel(
    const short* __restrict__ x, const int* __restrict__ row_src,
    const short* __restrict__ w, const int* __restrict__ offs,
    short* __restrict__ out, int N, int T, int E, int L, int C, int nct) {
  __shared__ short lds[2][4][IMG];  // [buffer][row img 0/1, col img 0/1]

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int c0 = (blockIdx.x % nct) * GT;

  int e, row0, row_end;
  if (!find_row_tile(offs, E, N, blockIdx.x / nct, lane, e, row0, row_end)) return;

  // the lane's rows of the two row images, fixed for the whole K loop; rows
  // past the group re-read its last row (never stored)
  int64_t xoff[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      xoff[i][j] = src_off(
          row_src[min(row0 + i * 64 + j * 32 + (lane >> 1), row_end - 1)], T,
          L, wid, lane);

  const int cimg0[2] = {c0, min(c0 + 64, C - 64)};
  const short* we = w + (int64_t)e * L * C;
  auto stage = [&](int s, int buf) {
    const int k = s * GK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_img_at(x + k, xoff[i], lds[buf][i], wid);
      stage_img(we + k, L, cimg0[i], C - 1, lds[buf][2 + i], wid, lane);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[ct][rt] = {0.f, 0.f, 0.f, 0.f};

  const int wr = wid >> 1, wc = wid & 1;
  const int nsteps = L / GK;
  stage(0, 0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) stage(s + 1, buf ^ 1);
    mma_step<false, false>(lds[buf][wr], lds[buf][2 + wc], acc, l15, lg, GK);
    __syncthreads();
  }

  const int col0 = c0 + wc * 64;
  if (col0 < C)
    store_quarter(acc, out, C, row0 + wr * 64, row_end, col0, l15, lg);
}

// dw[e] [M, K] = dy[rows of e]^T . x[row_src[rows of e]].  Grid and walk as
// moe_gemm_dw_kernel; the index loads run two steps ahead of the MFMAs.
__global__ void __launch_bounds__(256, 2) moe_gemm_dw_gather_kernel(
    const short* __restrict__ dy, const short* __restrict__ x,
    const int* __restrict__ row_src, const int* __restrict__ offs,
    short* __restrict__ dw, int N, int T, int E, int M, int K, int nmt,
    int nkt) {
  __shared__ short lds[2][4][IMG];  // [buffer][dy img 0/1, x img 0/1]

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const GroupBlock gb = xcd_remap(blockIdx.x, E, nmt * nkt);
  const int e = gb.gid;
  const int m0 = (gb.within / nkt) * GT;
  const int k0 = (gb.within % nkt) * GT;
  const int lo = offs_at(offs, e - 1, N);
  const int hi = max(offs_at(offs, e, N), lo);

  const int mimg0[2] = {m0, min(m0 + 64, M - 64)};
  const int kimg0[2] = {k0, min(k0 + 64, K - 64)};
  // the source tokens of the lane's two rows of step s, as loaded: nothing
  // is computed from them before the stage that uses them, so the load is
  // not waited for in the step that issues it.  A step past the end yields
  // the group's last row (hi > lo wherever this is called).
  auto load_src = [&](int s, int (&t)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      t[j] = row_src[min(lo + s * GK + j * 32 + (lane >> 1), hi - 1)];
  };
  auto stage = [&](int s, int buf, const int (&t)[2]) {
    const int r = lo + s * GK;
    const int64_t off[2] = {src_off(t[0], T, K, wid, lane),
                            src_off(t[1], T, K, wid, lane)};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_img(dy + mimg0[i], M, r, hi - 1, lds[buf][i], wid, lane);
      stage_img_at(x + kimg0[i], off, lds[buf][2 + i], wid);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[ct][rt] = {0.f, 0.f, 0.f, 0.f};

  const int wr = wid >> 1, wc = wid & 1;
  const int nsteps = (hi - lo + GK - 1) / GK;  // 0 for an empty expert
  int ahead[2] = {0, 0};  // tokens of the step after the staged one
  if (nsteps > 0) {
    int first[2];
    load_src(0, first);
    stage(0, 0, first);
    load_src(1, ahead);
  }
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    int next[2];
    if (s + 1 < nsteps) stage(s + 1, buf ^ 1, ahead);
    // unconditional (the row is clamped): a load under the branch would be
    // waited for where the branch ends, ahead of the MFMAs
    load_src(s + 2, next);
    mma_step<true, true>(lds[buf][wr], lds[buf][2 + wc], acc, l15, lg,
                         hi - lo - s * GK);
    __syncthreads();
    ahead[0] = next[0];
    ahead[1] = next[1];
  }

  const int col0 = k0 + wc * 64;
  if (col0 < K)
    store_quarter(acc, dw + (int64_t)e * M * K, K, m0 + wr * 64, M, col0, l15,
                  lg);
}

extern "C" {
void moe_row_src_launch(const int* dest, int* row_src, int64_t T, int k,
                        hipStream_t s) {
  if (T < 1) return;
  const int64_t want = (T + 255) / 256;
  hipLaunchKernelGGL(moe_row_src_kernel,
                     dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(256), 0,
                     s, dest, row_src, (int)T, k);
}

void moe_gemm_rows_gather_launch(const void* x, const int* row_src,
                                 const void* weight, const int* offs,
                                 void* out, int64_t N, int64_t T, int E, int M,
                                 int K, hipStream_t s) {
  if (N == 0 || T == 0) return;
  const int nct = (M + GT - 1) / GT;
  const int64_t nrt = (N + GT - 1) / GT + E;
  hipLaunchKernelGGL(moe_gemm_rows_gather_kernel,
                     dim3((uint32_t)(nrt * nct)), dim3(256), 0, s,
                     (const short*)x, row_src, (const short*)weight, offs,
                     (short*)out, (int)N, (int)T, E, K, M, nct);
}

void moe_gemm_dw_gather_launch(const void* dy, const void* x,
                               const int* row_src, const int* offs, void* dw,
                               int64_t N, int64_t T, int E, int M, int K,
                               hipStream_t s) {
  // without tokens every expert is empty: N = 0 makes the kernel store zeros
  const int nmt = (M + GT - 1) / GT, nkt = (K + GT - 1) / GT;
  hipLaunchKernelGGL(moe_gemm_dw_gather_kernel,
                     dim3((uint32_t)(E * nmt * nkt)), dim3(256), 0, s,
                     (const short*)dy, (const short*)x, row_src, offs,
                     (short*)dw, (int)(T == 0 ? 0 : N), (int)T, E, M, K, nmt,
                     nkt);
}
}
