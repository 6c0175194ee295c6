// Grouped GEMMs of the mixture-of-experts layer for gfx950: the three
// products of ops/moe.py's expert_mm and its backward, bf16 in, f32
// accumulation in v_mfma_f32_16x16x32_bf16, one rounding in the epilogue.
//
//   a [N, K] bf16, rows sorted by expert; weight [E, M, K] bf16; offs int32
//   [E], inclusive cumulative rows per expert, read on the device only.
//
//   forward "NT"  y[r, :]  = a[r, :]  . weight[e]^T   moe_gemm_rows_kernel<false>
//   dA      "NN"  da[r, :] = dy[r, :] . weight[e]     moe_gemm_rows_kernel<true>
//   dW            dw[e]    = dy[rows e]^T . a[rows e]  moe_gemm_dw_kernel
//
// One structure serves all three.  A 256-thread block owns a 128 x 128
// output tile, a wave a 64 x 64 quarter of it (16 C fragments, 64 f32
// accumulators per lane).  The output's ROW index travels through the MFMA's
// B operand and its COLUMN index through the A operand, so that a lane's C
// fragment (n = l15, m = lg*4 + r) holds 4 consecutive output columns of one
// row: an 8-byte store.  Per 64-deep contraction step the block stages four
// 64 x 64 st_idx images (two per operand, one per wave half) by LDS-DMA
// (global_load_lds), double-buffered and issued one step ahead, one barrier
// per step.  An operand whose contraction index is its column index (a and
// weight in the forward, dy in dA) is read from its image with b128 row
// reads; one whose contraction index is its row index (weight in dA, both
// operands in dW) comes out transposed through ds_read_b64_tr_b16
// (tr16_frag_st), as V does in attention: no transposed copy anywhere.
//
// Work list.  The row-grouped kernels cut every expert's rows into tiles of
// 128, so no tile straddles two experts; the host only knows the bound
// ceil(N / 128) + E on their number.  Every wave finds its block's tile
// itself: a lane takes two experts' tile counts from offs, one wave scan
// gives the running tile count, a ballot the owner.  Blocks past the real
// count exit.  Ragged tiles clamp their loads to the group's last row and
// mask their stores.  In dW the contraction runs over the group's rows: the
// block that owns an output tile walks all of them (no split-K, no atomics,
// every element of dw written exactly once, zeros for an empty expert), and
// rows past the end, which the clamped loads fill with copies of the last
// row, are zeroed in the dy fragments before the MFMA.
//
// The tile code (stage_img, mma_step, store_quarter, offs_at, find_row_tile)
// is in moe_gemm_tile.h, shared with moe_gemm_gather.hip.
//
// MFMA fragment maps: see attention_fwd.hip.
#include "moe_gemm_tile.h"
#include "launchers.h"

// out[r, :] = a[r, :] . op(weight[e]) for the rows r of group e.
//   TRANS_B = false: a [N, L], weight [E, C, L], out [N, C]  (forward)
//   TRANS_B = true : a [N, L], weight [E, L, C], out [N, C]  (dA; a is dy)
// L (contraction) and C (output columns) are multiples of 64.  Grid:
// nrt * nct blocks, nrt >= ceil(N / 128) + E, column tile fastest.  (Dealing
// chunks of 8 row tiles x all column tiles to one XCD measured within
// +-5 % per product and 0.7 % in sum at the Qwen3-30B-A3B layer shape, so
// the blocks keep their order: _hip/README.md.)
template <bool TRANS_B>
__global__ void __launch_bounds__(256, 2) moe_gemm_rows_kernel(
    const short* __restrict__ a, const short* __restrict__ w,
    const int* __restrict__ offs, short* __restrict__ out, int N, int E,
    int L, int C, int nct) {
  __shared__ short lds[2][4][IMG];  // [buffer][row img 0/1, col img 0/1]

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int c0 = (blockIdx.x % nct) * GT;

  int e, row0, row_end;
  if (!find_row_tile(offs, E, N, blockIdx.x / nct, lane, e, row0, row_end)) return;

  // column images past C re-stage the last 64 columns (never stored)
  const int cimg0[2] = {c0, min(c0 + 64, C - 64)};
  const short* we = w + (int64_t)e * L * C;
  auto stage = [&](int s, int buf) {
    const int k = s * GK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_img(a + k, L, row0 + i * 64, row_end - 1, lds[buf][i], wid, lane);
      if (TRANS_B)
        stage_img(we + cimg0[i], C, k, L - 1, lds[buf][2 + i], wid, lane);
      else
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
    mma_step<false, TRANS_B>(lds[buf][wr], lds[buf][2 + wc], acc, l15, lg, GK);
    __syncthreads();
  }

  const int col0 = c0 + wc * 64;
  if (col0 < C)
    store_quarter(acc, out, C, row0 + wr * 64, row_end, col0, l15, lg);
}

// dw[e] [M, K] = dy[rows of e]^T . a[rows of e]: block (e, m tile, k tile)
// walks the expert's rows 64 at a time.  Grid E * nmt * nkt, an expert's
// tiles dealt to one XCD (xcd_remap) so that its rows of dy and a stay in
// that L2.
__global__ void __launch_bounds__(256, 2) moe_gemm_dw_kernel(
    const short* __restrict__ dy, const short* __restrict__ a,
    const int* __restrict__ offs, short* __restrict__ dw, int N, int E, int M,
    int K, int nmt, int nkt) {
  __shared__ short lds[2][4][IMG];  // [buffer][dy img 0/1, a img 0/1]

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
  auto stage = [&](int s, int buf) {
    const int r = lo + s * GK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stage_img(dy + mimg0[i], M, r, hi - 1, lds[buf][i], wid, lane);
      stage_img(a + kimg0[i], K, r, hi - 1, lds[buf][2 + i], wid, lane);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[ct][rt] = {0.f, 0.f, 0.f, 0.f};

  const int wr = wid >> 1, wc = wid & 1;
  const int nsteps = (hi - lo + GK - 1) / GK;  // 0 for an empty expert
  if (nsteps > 0) stage(0, 0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) stage(s + 1, buf ^ 1);
    mma_step<true, true>(lds[buf][wr], lds[buf][2 + wc], acc, l15, lg,
                         hi - lo - s * GK);
    __syncthreads();
  }

  const int col0 = k0 + wc * 64;
  if (col0 < K)
    store_quarter(acc, dw + (int64_t)e * M * K, K, m0 + wr * 64, M, col0, l15,
                  lg);
}

extern "C" void moe_gemm_rows_launch(const void* a, const void* weight,
                                     const int* offs, void* out, int64_t N,
                                     int E, int M, int K, int trans_b,
                                     hipStream_t s) {
  if (N == 0) return;
  const int L = trans_b ? M : K, C = trans_b ? K : M;
  const int nct = (C + GT - 1) / GT;
  const int64_t nrt = (N + GT - 1) / GT + E;
  auto kern = trans_b ? moe_gemm_rows_kernel<true>
                      : moe_gemm_rows_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((uint32_t)(nrt * nct)), dim3(256), 0, s,
                     (const short*)a, (const short*)weight, offs, (short*)out,
                     (int)N, E, L, C, nct);
}

extern "C" void moe_gemm_dw_launch(const void* dy, const void* a,
                                   const int* offs, void* dw, int64_t N, int E,
                                   int M, int K, hipStream_t s) {
  const int nmt = (M + GT - 1) / GT, nkt = (K + GT - 1) / GT;
  hipLaunchKernelGGL(moe_gemm_dw_kernel, dim3((uint32_t)(E * nmt * nkt)),
                     dim3(256), 0, s, (const short*)dy, (const short*)a, offs,
                     (short*)dw, (int)N, E, M, K, nmt, nkt);
}
