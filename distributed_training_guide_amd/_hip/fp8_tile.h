// The 64x64 cast tile of the e4m3 kernels (fp8_quant.hip, fp8_delayed.hip):
// one wave per tile, a 4x16 patch of bf16 per lane; the layout, the LDS image
// and its swizzle are described at the top of fp8_quant.hip.  A kernel fills
// the patch (a plain load, or SwiGLU of two loads), then calls
// fp8_patch_store for the inside lanes and fp8_image_flush for the whole wave.
#pragma once
#include "common.h"

#define FP8_E4M3_MAX 448.0f
#define FP8_AMAX_FLOOR 1e-12f
#define FP8_TILE 64

__device__ __forceinline__ uint32_t wave_reduce_umax(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, WAVE);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ float fp8_scale_clamp(short bits, float scale) {
  float v = bf2f(bits) * scale;
  v = v > FP8_E4M3_MAX ? FP8_E4M3_MAX : v;
  v = v < -FP8_E4M3_MAX ? -FP8_E4M3_MAX : v;
  return v;
}

// four e4m3 in one dword, a in the lowest byte
__device__ __forceinline__ uint32_t pack4_e4m3(float a, float b, float c,
                                               float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

// A lane's place in its block's tile of an [R, C] tensor.
struct Fp8Tile {
  int lane, cb, rg;    // cb: block of 16 columns, rg: group of 4 rows
  int tile_r, tile_c;  // the tile's first row and column
  int r0, c0;          // the patch's first row and column
  bool inside;
};

__device__ __forceinline__ Fp8Tile fp8_tile(int R, int C, int tiles_c) {
  Fp8Tile t;
  t.lane = threadIdx.x;
  t.cb = t.lane & 3;
  t.rg = t.lane >> 2;
  const int bid = (int)blockIdx.x;
  t.tile_r = (bid / tiles_c) * FP8_TILE;
  t.tile_c = (bid % tiles_c) * FP8_TILE;
  t.r0 = t.tile_r + t.rg * 4;
  t.c0 = t.tile_c + t.cb * 16;
  t.inside = t.r0 < R && t.c0 < C;
  return t;
}

// Scale, clamp and convert the patch; the row-major output goes out from
// registers, the transposed one into `image` ([col in tile][row in tile / 4]
// dwords of 4 e4m3 down the rows, FP8_TILE * 16 dwords, 16 B aligned).
template <bool ROW, bool TR>
__device__ __forceinline__ void fp8_patch_store(const s16x8 (&raw)[4][2],
                                                float scale, const Fp8Tile& t,
                                                uint32_t* image,
                                                uint8_t* __restrict__ q,
                                                int C) {
  float v[4][16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[i][j] = fp8_scale_clamp(raw[i][0][j], scale);
      v[i][8 + j] = fp8_scale_clamp(raw[i][1][j], scale);
    }
  if constexpr (ROW) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u32x4 w;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        w[m] = pack4_e4m3(v[i][4 * m], v[i][4 * m + 1], v[i][4 * m + 2],
                          v[i][4 * m + 3]);
      *reinterpret_cast<u32x4*>(q + (int64_t)(t.r0 + i) * C + t.c0) = w;
    }
  }
  if constexpr (TR) {
    const int d = t.rg ^ ((t.cb & 1) << 3);
#pragma unroll
    for (int k = 0; k < 16; ++k)
      image[(t.cb * 16 + k) * 16 + d] =
          pack4_e4m3(v[0][k], v[1][k], v[2][k], v[3][k]);
  }
}

// The whole wave: the image back out as 16 B runs of qt [C, R] rows.
__device__ __forceinline__ void fp8_image_flush(const uint32_t* image,
                                                const Fp8Tile& t,
                                                uint8_t* __restrict__ qt,
                                                int R, int C) {
  __syncthreads();
  const int run = t.lane & 3;  // 16 tile rows = one 16 B run of a qt row
  const int gr = t.tile_r + run * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int col = i * 16 + (t.lane >> 2);  // column block i
    const int gc = t.tile_c + col;
    if (gc < C && gr < R) {
      const int slot = run ^ ((i & 1) << 1);
      const u32x4 w =
          *reinterpret_cast<const u32x4*>(&image[col * 16 + slot * 4]);
      *reinterpret_cast<u32x4*>(qt + (int64_t)gc * R + gr) = w;
    }
  }
}

// Largest sign-cleared bf16 bit pattern of the patch: an integer max is
// exact and a NaN (above 0x7f80) wins.  The two 16-bit halves of each dword
// are folded separately, as in fp8_amax_partials_kernel.
__device__ __forceinline__ uint32_t fp8_patch_umax(const s16x8 (&raw)[4][2]) {
  uint32_t mlo = 0, mhi = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u32x4 v = __builtin_bit_cast(u32x4, raw[i][h]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo = v[j] & 0x7fffu, hi = (v[j] >> 16) & 0x7fffu;
        mlo = lo > mlo ? lo : mlo;
        mhi = hi > mhi ? hi : mhi;
      }
    }
  return mlo > mhi ? mlo : mhi;
}
