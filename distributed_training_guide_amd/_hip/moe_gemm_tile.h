// The 128 x 128 output tile of the grouped expert GEMMs (moe_gemm.hip,
// moe_gemm_gather.hip, moe_gemm_swiglu.hip): the LDS-DMA staging of one
// 64 x 64 st_idx image (by row range or through a row index), the 64-deep
// MFMA step of a wave's 64 x 64 quarter, its store, and the search of the
// expert-major list of row tiles.  The structure is described at the top of
// moe_gemm.hip.
#pragma once
#include "attention_common.h"

constexpr int GT = 128;       // rows and columns of an output tile
constexpr int GK = 64;        // contraction step
constexpr int IMG = 64 * 64;  // shorts of one 64 x 64 st_idx image

// Stages rows [row0, row0 + 64) x 64 columns of a row-major bf16 tensor (g
// points at the first column) into one st_idx image: the chunk mapping of
// stage_tile_pair (attention_common.h), two chunks per wave.  Rows past
// row_last re-read row_last (in bounds; the callers mask them).  The LDS
// address is the image base plus a multiple of wid and the unrolled i,
// nothing lane-derived.
__device__ __forceinline__ void stage_img(const short* g, int64_t stride,
                                          int row0, int row_last, short* img,
                                          int wid, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ch = wid * 2 + i;
    const int row = min(row0 + (ch & 1) * 32 + (lane >> 1), row_last);
    const int64_t goff =
        (int64_t)row * stride + (ch >> 1) * 16 + (lane & 1) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(g + goff),
        (LDS_AS unsigned int*)(img + ch * 512), 16, 0, 0);
  }
}

// A lane's element offset into x for the source token `t` of a sorted row,
// clamped into [0, T): the token's row plus the lane's 8 columns of the
// wave's 16-column subtile.
__device__ __forceinline__ int64_t src_off(int t, int T, int64_t stride,
                                           int wid, int lane) {
  return (int64_t)min(max(t, 0), T - 1) * stride + wid * 16 + (lane & 1) * 8;
}

// stage_img with the lane's two rows given as element offsets from g: chunk
// wid*2 + j lands at the same place of the image.
__device__ __forceinline__ void stage_img_at(const short* g,
                                             const int64_t (&off)[2],
                                             short* img, int wid) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(g + off[j]),
        (LDS_AS unsigned int*)(img + (wid * 2 + j) * 512), 16, 0, 0);
}

// One 64-deep contraction step of a wave's 64 x 64 quarter.  rimg / cimg are
// the images of the operands that carry the output's row / column index;
// *_TR says the image's rows are the contraction index (transposed read).
// kvalid < 64 (R_TR only) zeroes the row operand's contraction rows from
// kvalid on.  All 32 MFMAs are issued unconditionally.
template <bool R_TR, bool C_TR>
__device__ __forceinline__ void mma_step(const short* rimg, const short* cimg,
                                         f32x4 (&acc)[4][4], int l15, int lg,
                                         int kvalid) {
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    const int k0 = kc * 32 + lg * 8;
    bf16x8 rf[4], cf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if constexpr (R_TR)
        rf[t] = tr16_frag_st(rimg, k0, t * 16, l15);
      else
        rf[t] = *reinterpret_cast<const bf16x8*>(
            rimg + st_idx(t * 16 + l15, k0));
      if constexpr (C_TR)
        cf[t] = tr16_frag_st(cimg, k0, t * 16, l15);
      else
        cf[t] = *reinterpret_cast<const bf16x8*>(
            cimg + st_idx(t * 16 + l15, k0));
    }
    if constexpr (R_TR) {
      if (kvalid < GK) {  // operand masking only; the MFMAs stay outside
        u32x4 m;
#pragma unroll
        for (int p = 0; p < 4; ++p)
          m[p] = (k0 + 2 * p < kvalid ? 0x0000ffffu : 0u) |
                 (k0 + 2 * p + 1 < kvalid ? 0xffff0000u : 0u);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          rf[t] = __builtin_bit_cast(
              bf16x8, __builtin_bit_cast(u32x4, rf[t]) & m);
      }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[ct][rt] = mfma16(cf[ct], rf[rt], acc[ct][rt]);
  }
}

// mma_step<false, false> with the wave's column fragments taken from two
// images: ct 0, 1 from rows crow + ct*16 + l15 of cimg_a, ct 2, 3 from the
// same rows of cimg_b.  With the gate rows of a weight in cimg_a and the
// matching up rows in cimg_b (moe_gemm_swiglu.hip) a lane holds g in
// acc[ct][rt] and u in acc[ct + 2][rt] of the same (row, column).
__device__ __forceinline__ void mma_step_pair(const short* rimg,
                                              const short* cimg_a,
                                              const short* cimg_b, int crow,
                                              f32x4 (&acc)[4][4], int l15,
                                              int lg) {
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    const int k0 = kc * 32 + lg * 8;
    bf16x8 rf[4], cf[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      rf[t] = *reinterpret_cast<const bf16x8*>(
          rimg + st_idx(t * 16 + l15, k0));
      cf[t] = *reinterpret_cast<const bf16x8*>(
          (t < 2 ? cimg_a : cimg_b) + st_idx(crow + (t & 1) * 16 + l15, k0));
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[ct][rt] = mfma16(cf[ct], rf[rt], acc[ct][rt]);
  }
}

// Stores a wave's quarter: C fragment [ct][rt] holds output row
// rt*16 + l15, columns ct*16 + lg*4 + r of the quarter at (row0, col0).
// Rows from row_end on are not written.
__device__ __forceinline__ void store_quarter(const f32x4 (&acc)[4][4],
                                              short* out, int64_t stride,
                                              int row0, int row_end, int col0,
                                              int l15, int lg) {
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int row = row0 + rt * 16 + l15;
    if (row >= row_end) continue;
    short* op = out + (int64_t)row * stride + col0 + lg * 4;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      s16x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = f2bf(acc[ct][rt][r]);
      *reinterpret_cast<s16x4*>(op + ct * 16) = v;
    }
  }
}

// offs[e] as the kernels use it: clamped into [0, N], so that a table
// outside the contract cannot move a load or a store out of bounds.
__device__ __forceinline__ int offs_at(const int* offs, int e, int N) {
  return e < 0 ? 0 : min(max(offs[e], 0), N);
}

// The row tile `tile` of the expert-major list of 128-row tiles: lane l
// counts the tiles of experts 2l and 2l + 1 (E <= 128), an inclusive wave
// scan numbers them, the one lane whose range holds `tile` answers.
// Wave-uniform results; false when `tile` is past the list.
__device__ __forceinline__ bool find_row_tile(const int* offs, int E, int N,
                                              int tile, int lane, int& e,
                                              int& row0, int& row_end) {
  const int e0 = 2 * lane;
  // experts past E - 1 count as empty; a non-monotone table as empty groups
  const int lo = offs_at(offs, min(e0, E) - 1, N);
  const int mid = max(offs_at(offs, min(e0 + 1, E) - 1, N), lo);
  const int hi = max(offs_at(offs, min(e0 + 2, E) - 1, N), mid);
  const int t0 = (mid - lo + GT - 1) / GT, t1 = (hi - mid + GT - 1) / GT;
  int incl = t0 + t1;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off, WAVE);
    if (lane >= off) incl += up;
  }
  const int excl = incl - t0 - t1;
  const unsigned long long owner = __ballot(tile >= excl && tile < incl);
  if (owner == 0) return false;
  const int src = __ffsll(owner) - 1;
  const bool second = tile >= excl + t0;
  const int my_e = second ? e0 + 1 : e0;
  const int my_row0 = second ? mid + (tile - excl - t0) * GT
                             : lo + (tile - excl) * GT;
  const int my_end = second ? hi : mid;
  e = __builtin_amdgcn_readfirstlane(__shfl(my_e, src, WAVE));
  row0 = __builtin_amdgcn_readfirstlane(__shfl(my_row0, src, WAVE));
  row_end = __builtin_amdgcn_readfirstlane(__shfl(my_end, src, WAVE));
  return true;
}
