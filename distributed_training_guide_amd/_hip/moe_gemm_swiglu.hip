// Weighted SwiGLU in the epilogues of the expert GEMMs for gfx950: the
// router weight is applied to h before the down projection,
//
//   sum_j w[t, j] * (h_r . Wd^T) = sum_j ((w_r * h_r) . Wd^T),
//
// so the combine is an unweighted k-way sum whose backward needs nothing
// saved, and the router-weight gradient is a row dot product over I columns
// that is taken while dh' is still in accumulators.
//
//   x [T, H] bf16; row_src int32 [N] (moe_row_src_kernel); w_row f32 [N], the
//   router weight of every sorted row (moe_row_w_kernel); gate_up [E, 2I, H];
//   down [E, H, I]; offs int32 [E].  I is a multiple of 64.
//
//   forward   gu[r, :] = x[row_src[r]] . gate_up[e]^T            (bf16, saved)
//             h'[r, c] = bf16(w_row[r] * silu(gu[r, c]) * gu[r, I + c])
//                                                moe_gemm_gu_swiglu_kernel
//   backward  dh' = dyp . down[e]                (accumulators only)
//             dgu[r, c]     = w dh' u sig (1 + g (1 - sig))
//             dgu[r, I + c] = w dh' silu(g)
//             dwp[r, p]     = sum over the columns of part p of dh' silu(g) u
//                                                moe_gemm_da_swiglu_kernel
//             dw_topk[s] = sum_p dwp[dest[s], p]    moe_dw_finish_kernel
//
// Tiling, work search, DMA staging, double buffering and the MFMA step are
// those of moe_gemm.hip / moe_gemm_gather.hip (moe_gemm_tile.h).
//
// Forward.  A block owns 128 rows x 64 HIDDEN columns [c0, c0 + 64): its two
// column-operand images of a K-step are the gate rows [c0, c0 + 64) and the
// up rows [I + c0, I + c0 + 64) of gate_up[e], so the block count is that of
// the 2I / 128 column tiles of the plain GEMM.  Wave (wr, wc) takes rows
// wr*64.. and the hidden columns c0 + wc*32..: C fragments 0, 1 from the gate
// image, 2, 3 from the same rows of the up image (mma_step_pair).  A lane
// then holds g in acc[ct][rt] and u in acc[ct + 2][rt] of the same (row,
// column): the activation needs no exchange between lanes or waves.  Every
// accumulator sees the MFMAs of moe_gemm_rows_gather_kernel in their order,
// so gu is that kernel's bits.  h' is formed from the ROUNDED g and u, the
// values the backward recomputes from.
//
// Backward.  The TRANS_B tile of moe_gemm_rows_kernel over [N, I].  A lane
// loads g and u of its 4 consecutive columns from gu (8 bytes each).  The row
// partial of dw (without w) is summed in the lane over its 4 x 4 values, then
// over the four lane groups that share a row (two shuffles), and stored by
// plain stores: one f32 per row per (column tile, wave column half),
// dwp [N, 2 * ceil(I / 128)].  Every entry of a real row is written, a half
// past I as zero, nothing is cleared, and the finishing kernel adds a row's
// entries in index order: no atomics, bitwise reproducible.
#include "moe_gemm_tile.h"
#include "launchers.h"
#include "silu.h"

constexpr int RW_MAX_K = 8;

// w_row[dest[t*k + j]] = topk_w[t, j]: moe_row_src_kernel's walk with the
// weight as the value.  dest is a permutation of [0, T*k): every element is
// written once, no atomics, nothing cleared.  A value outside is dropped.
__global__ void __launch_bounds__(256) moe_row_w_kernel(
    const int* __restrict__ dest, const float* __restrict__ topk_w,
    float* __restrict__ w_row, int T, int k) {
  const int N = T * k;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += gridDim.x * 256) {
    const int* d = dest + (int64_t)t * k;
    const float* w = topk_w + (int64_t)t * k;
    int r[RW_MAX_K];  // all loads first; slots past k re-read the last one
    float v[RW_MAX_K];
#pragma unroll
    for (int j = 0; j < RW_MAX_K; ++j) {
      r[j] = d[min(j, k - 1)];
      v[j] = w[min(j, k - 1)];
    }
#pragma unroll
    for (int j = 0; j < RW_MAX_K; ++j)
      if (j < k && (unsigned)r[j] < (unsigned)N) w_row[r[j]] = v[j];
  }
}

// gu [N, 2I] and hw [N, I] from x [T, L] through row_src, weight [E, 2I, L].
// Grid: nrt * nct blocks, nct = I / 64, nrt >= ceil(N / 128) + E, column tile
// fastest.
__global__ void __launch_bounds__(256, 2) moe_gemm_gu_swiglu_kernel(
    const short* __restrict__ x, const int* __restrict__ row_src,
    const float* __restrict__ w_row, const short* __restrict__ w,
    const int* __restrict__ offs, short* __restrict__ gu,
    short* __restrict__ hw, int N, int T, int E, int L, int I, int nct) {
  __shared__ short lds[2][4][IMG];  // [buffer][row img 0/1, gate img, up img]

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int c0 = (blockIdx.x % nct) * 64;

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

  const int C = 2 * I;
  const short* we = w + (int64_t)e * L * C;
  auto stage = [&](int s, int buf) {
    const int k = s * GK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_img_at(x + k, xoff[i], lds[buf][i], wid);
      stage_img(we + k, L, i * I + c0, C - 1, lds[buf][2 + i], wid, lane);
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
    mma_step_pair(lds[buf][wr], lds[buf][2], lds[buf][3], wc * 32, acc, l15,
                  lg);
    __syncthreads();
  }

  const int col0 = c0 + wc * 32 + lg * 4;  // of [0, I)
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int row = row0 + wr * 64 + rt * 16 + l15;
    if (row >= row_end) continue;
    const float wv = w_row[row];
    short* gp = gu + (int64_t)row * C + col0;
    short* hp = hw + (int64_t)row * I + col0;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      s16x4 g, u, h;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        g[r] = f2bf(acc[ct][rt][r]);
        u[r] = f2bf(acc[ct + 2][rt][r]);
        h[r] = f2bf(wv * silu_mul_f32(bf2f(g[r]), bf2f(u[r])));
      }
      *reinterpret_cast<s16x4*>(gp + ct * 16) = g;
      *reinterpret_cast<s16x4*>(gp + I + ct * 16) = u;
      *reinterpret_cast<s16x4*>(hp + ct * 16) = h;
    }
  }
}

// dgu [N, 2I] and dwp [N, 2 * nct] from dyp [N, L], down [E, L, I], the saved
// gu [N, 2I] and w_row.  Grid as moe_gemm_rows_kernel<true> with C = I.
__global__ void __launch_bounds__(256, 2) moe_gemm_da_swiglu_kernel(
    const short* __restrict__ dyp, const short* __restrict__ w,
    const short* __restrict__ gu, const float* __restrict__ w_row,
    const int* __restrict__ offs, short* __restrict__ dgu,
    float* __restrict__ dwp, int N, int E, int L, int I, int nct) {
  __shared__ short lds[2][4][IMG];  // [buffer][row img 0/1, col img 0/1]

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int ctile = blockIdx.x % nct;
  const int c0 = ctile * GT;

  int e, row0, row_end;
  if (!find_row_tile(offs, E, N, blockIdx.x / nct, lane, e, row0, row_end)) return;

  // a column image past I re-stages the last 64 columns; its wave neither
  // stores them nor adds them to the row partial
  const int cimg0[2] = {c0, min(c0 + 64, I - 64)};
  const short* we = w + (int64_t)e * L * I;
  auto stage = [&](int s, int buf) {
    const int k = s * GK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_img(dyp + k, L, row0 + i * 64, row_end - 1, lds[buf][i], wid, lane);
      stage_img(we + cimg0[i], I, k, L - 1, lds[buf][2 + i], wid, lane);
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
    mma_step<false, true>(lds[buf][wr], lds[buf][2 + wc], acc, l15, lg, GK);
    __syncthreads();
  }

  const int col0 = c0 + wc * 64;
  const bool live = col0 < I;  // wave-uniform
  const int C = 2 * I;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int row = row0 + wr * 64 + rt * 16 + l15;
    const bool real = row < row_end;
    float part = 0.f;
    if (live && real) {
      const float wv = w_row[row];
      const short* gp = gu + (int64_t)row * C + col0 + lg * 4;
      short* dp = dgu + (int64_t)row * C + col0 + lg * 4;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const s16x4 g = *reinterpret_cast<const s16x4*>(gp + ct * 16);
        const s16x4 u = *reinterpret_cast<const s16x4*>(gp + I + ct * 16);
        s16x4 og, ou;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gv = bf2f(g[r]), uv = bf2f(u[r]);
          const float sig = 1.0f / (1.0f + __expf(-gv));
          const float sx = gv * sig;
          const float d = acc[ct][rt][r];
          part += d * (sx * uv);
          const float dd = wv * d;
          ou[r] = f2bf(dd * sx);
          og[r] = f2bf(dd * uv * sig * (1.0f + gv * (1.0f - sig)));
        }
        *reinterpret_cast<s16x4*>(dp + ct * 16) = og;
        *reinterpret_cast<s16x4*>(dp + I + ct * 16) = ou;
      }
    }
    // the four lane groups hold the four 4-column slices of the same row
    part += __shfl_xor(part, 16, WAVE);
    part += __shfl_xor(part, 32, WAVE);
    if (lg == 0 && real)
      dwp[(int64_t)row * (2 * nct) + ctile * 2 + wc] = part;
  }
}

// dw_topk[s] = sum_p dwp[dest[s], p], added in index order.
__global__ void __launch_bounds__(256) moe_dw_finish_kernel(
    const float* __restrict__ dwp, const int* __restrict__ dest,
    float* __restrict__ dw_topk, int N, int P) {
  for (int s = blockIdx.x * 256 + threadIdx.x; s < N; s += gridDim.x * 256) {
    const int r = dest[s];
    float sum = 0.f;
    if ((unsigned)r < (unsigned)N) {
      const float* p = dwp + (int64_t)r * P;
      for (int i = 0; i < P; ++i) sum += p[i];
    }
    dw_topk[s] = sum;
  }
}

extern "C" {
void moe_row_w_launch(const int* dest, const float* topk_w, float* w_row,
                      int64_t T, int k, hipStream_t s) {
  if (T < 1) return;
  const int64_t want = (T + 255) / 256;
  hipLaunchKernelGGL(moe_row_w_kernel,
                     dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(256), 0,
                     s, dest, topk_w, w_row, (int)T, k);
}

void moe_gemm_gu_swiglu_launch(const void* x, const int* row_src,
                               const float* w_row, const void* gate_up,
                               const int* offs, void* gu, void* hw, int64_t N,
                               int64_t T, int E, int I, int K, hipStream_t s) {
  if (N == 0 || T == 0) return;
  const int nct = I / 64;
  const int64_t nrt = (N + GT - 1) / GT + E;
  hipLaunchKernelGGL(moe_gemm_gu_swiglu_kernel, dim3((uint32_t)(nrt * nct)),
                     dim3(256), 0, s, (const short*)x, row_src, w_row,
                     (const short*)gate_up, offs, (short*)gu, (short*)hw,
                     (int)N, (int)T, E, K, I, nct);
}

int moe_dw_parts(int I) { return 2 * ((I + GT - 1) / GT); }

void moe_gemm_da_swiglu_launch(const void* dyp, const void* down,
                               const void* gu, const float* w_row,
                               const int* offs, const int* dest, void* dgu,
                               float* dwp, float* dw_topk, int64_t N, int E,
                               int H, int I, hipStream_t s) {
  if (N == 0) return;
  const int nct = (I + GT - 1) / GT;
  const int64_t nrt = (N + GT - 1) / GT + E;
  hipLaunchKernelGGL(moe_gemm_da_swiglu_kernel, dim3((uint32_t)(nrt * nct)),
                     dim3(256), 0, s, (const short*)dyp, (const short*)down,
                     (const short*)gu, w_row, offs, (short*)dgu, dwp, (int)N,
                     E, H, I, nct);
  const int64_t want = (N + 255) / 256;
  hipLaunchKernelGGL(moe_dw_finish_kernel,
                     dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(256), 0,
                     s, dwp, dest, dw_topk, (int)N, 2 * nct);
}
}
