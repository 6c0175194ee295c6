// Tensor-wise dynamic FP8 quantisation for gfx950: the memory-bound work
// around the hipBLASLt FP8 GEMMs of ops/fp8_linear.py.  OCP e4m3 (torch's
// float8_e4m3fn, largest finite value 448) for every operand.
//
// Two passes over a contiguous bf16 [R, C] tensor:
//
//   1. fp8_amax_scale_launch: amax, then
//        scale = 448 / max(amax, 1e-12)      inv_scale = max(amax, 1e-12) / 448
//      Same structure as grad_norm.hip: every block writes one partial with an
//      ordinary store, a single block folds them; no atomics, no pre-zeroed
//      buffer, the two fp32 results stay on the device.  The max is taken on
//      the bf16 bit pattern with the sign cleared: an integer max is exact,
//      and a NaN (above 0x7f80) wins.  Both quotients are IEEE divisions and
//      each is the definition of its value (1/scale != inv_scale in general).
//      The floor makes an all-zero tensor quantise to zeros.  The floor is a
//      compare, not fmaxf, so a non-finite input is not hidden: a NaN amax
//      gives NaN scales and an all-NaN result, an inf amax gives scale 0 and
//      inv_scale inf (finite elements become 0, the inf elements NaN).
//
//   2. fp8_cast_transpose_launch: q = cvt_rne(clamp(float(x) * scale, +-448)),
//      written row-major [R, C], transposed [C, R], or both (a null pointer
//      drops an output, as in norm_*_launch); x is read once and `scale` comes
//      from device memory.  One fp32 multiply, a clamp and v_cvt_pk_fp8_f32
//      per element: defined bit for bit.  The clamp is explicit (torch's own
//      cast gives NaN above 448) and written as two compares so that NaN
//      stays NaN; v_med3_f32 would turn it into -448.
//
// Cast kernel layout.  One wave owns a 64x64 tile.  Lane l holds rows
// 4*(l>>2) .. +3 and columns 16*(l&3) .. +15: eight 16 B loads, 64 values.
//   - row-major output straight from registers: four e4m3 per dword with two
//     v_cvt_pk_fp8_f32, sixteen columns = one 16 B store per row;
//   - transposed output: the same values packed down the rows instead (the
//     lane's 4 rows of one column = one dword, no byte shuffles), written to
//     a [64 cols][64 rows] byte image in LDS with ds_write_b32, read back as
//     16 B runs of one column and stored 16 B wide, 64 B per qt row.
// LDS banks: the image's rows are 16 dwords and a lane's dword index is its
// row group (0..15), so the 32 lanes of a ds_write_b32 group (8 row groups x
// 4 column blocks, the blocks 16 image rows = 256 dwords apart) would share
// 8 banks 4 ways.  The two 32 B halves of an image row swap for odd column
// blocks (`^ 8` on the dword index): 2 ways, which a ds_write_b32's own issue
// time absorbs (the compiler pairs the stores into ds_write2_b32).  The
// ds_read_b128 groups each cover four image rows that differ mod 4, i.e. 256
// distinct bytes: conflict-free.  Row padding cannot do this: rows must stay
// 16 B aligned for the b128 reads and every such stride puts column blocks on
// the same banks.  Counters agree: per tile 12 LDS instructions, 80 LDS-array
// cycles, 32 of them SQ_LDS_BANK_CONFLICT = the 2-way stores and nothing else,
// against the well over 1000 cycles a CU's share of HBM needs for the tile.
//
// R % 16 == 0 and C % 16 == 0 (the FP8 GEMM's own requirement, checked by
// the binding), so a lane's 4x16 patch and every 16 B run is entirely inside
// or outside the tensor; tiles may hang over either edge.
#include "common.h"
#include "launchers.h"

#define FP8_E4M3_MAX 448.0f
#define FP8_AMAX_FLOOR 1e-12f
#define FP8_TILE 64

// ---------------------------------------------------------------- amax
__device__ __forceinline__ uint32_t wave_reduce_umax(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// 256 threads; the result is valid in thread 0
__device__ __forceinline__ uint32_t block4_umax(uint32_t v, uint32_t* sh) {
  v = wave_reduce_umax(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t a = sh[0] > sh[1] ? sh[0] : sh[1];
  const uint32_t b = sh[2] > sh[3] ? sh[2] : sh[3];
  return a > b ? a : b;
}

// partials[block] = max over the block's 8-element vectors of |bits|
__global__ void __launch_bounds__(256) fp8_amax_partials_kernel(
    const short* __restrict__ x, int64_t n8, uint32_t* __restrict__ partials) {
  __shared__ uint32_t sh[4];
  // two lanes of 16 bits per dword, folded separately: no cross-lane carries
  uint32_t mlo = 0, mhi = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
#pragma unroll 4
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8;
       i += stride) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + i * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t lo = v[j] & 0x7fffu, hi = (v[j] >> 16) & 0x7fffu;
      mlo = lo > mlo ? lo : mlo;
      mhi = hi > mhi ? hi : mhi;
    }
  }
  const uint32_t m = block4_umax(mlo > mhi ? mlo : mhi, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// <<<1, 256>>>: fold the partials, write out[0] = scale, out[1] = inv_scale
__global__ void __launch_bounds__(256) fp8_scale_final_kernel(
    const uint32_t* __restrict__ partials, int nparts,
    float* __restrict__ out) {
  __shared__ uint32_t sh[4];
  uint32_t m = 0;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    const uint32_t p = partials[i];
    m = p > m ? p : m;
  }
  m = block4_umax(m, sh);
  if (threadIdx.x == 0) {
    const float amax = bf2f((short)m);
    // a compare, not fmaxf: a NaN amax stays NaN (torch.clamp does the same)
    const float a = amax < FP8_AMAX_FLOOR ? FP8_AMAX_FLOOR : amax;
    out[0] = __fdiv_rn(FP8_E4M3_MAX, a);
    out[1] = __fdiv_rn(a, FP8_E4M3_MAX);
  }
}

// ---------------------------------------------------------------- cast
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

template <bool ROW, bool TR>
__global__ void __launch_bounds__(64) fp8_cast_transpose_kernel(
    const short* __restrict__ x, const float* __restrict__ scale_p,
    uint8_t* __restrict__ q, uint8_t* __restrict__ qt, int R, int C,
    int tiles_c) {
  // [col in tile][row in tile / 4] dwords of 4 e4m3 down the rows
  __shared__ __attribute__((aligned(16))) uint32_t image[FP8_TILE * 16];
  const int lane = threadIdx.x;
  const int cb = lane & 3;   // block of 16 columns
  const int rg = lane >> 2;  // group of 4 rows
  const int bid = (int)blockIdx.x;
  const int tile_r = (bid / tiles_c) * FP8_TILE;
  const int tile_c = (bid % tiles_c) * FP8_TILE;
  const int r0 = tile_r + rg * 4;
  const int c0 = tile_c + cb * 16;
  const bool inside = r0 < R && c0 < C;

  if (inside) {
    const float scale = *scale_p;
    s16x8 raw[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const short* src = x + (int64_t)(r0 + i) * C + c0;
      raw[i][0] = *reinterpret_cast<const s16x8*>(src);
      raw[i][1] = *reinterpret_cast<const s16x8*>(src + 8);
    }
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
        *reinterpret_cast<u32x4*>(q + (int64_t)(r0 + i) * C + c0) = w;
      }
    }
    if constexpr (TR) {
      const int d = rg ^ ((cb & 1) << 3);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        image[(cb * 16 + k) * 16 + d] =
            pack4_e4m3(v[0][k], v[1][k], v[2][k], v[3][k]);
    }
  }
  if constexpr (TR) {
    __syncthreads();
    const int run = lane & 3;  // 16 tile rows = one 16 B run of a qt row
    const int gr = tile_r + run * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = i * 16 + (lane >> 2);  // column block i
      const int gc = tile_c + col;
      if (gc < C && gr < R) {
        const int slot = run ^ ((i & 1) << 1);
        const u32x4 w =
            *reinterpret_cast<const u32x4*>(&image[col * 16 + slot * 4]);
        *reinterpret_cast<u32x4*>(qt + (int64_t)gc * R + gr) = w;
      }
    }
  }
}

extern "C" {
int fp8_amax_blocks(int64_t numel) {
  const int64_t want = (numel / 8 + 1023) / 1024;  // >= 4 vectors a thread
  return (int)(want < 1 ? 1 : want < 2048 ? want : 2048);
}

void fp8_amax_scale_launch(const void* x, int64_t numel, void* partials,
                           float* scales, hipStream_t s) {
  const int nblocks = fp8_amax_blocks(numel);
  hipLaunchKernelGGL(fp8_amax_partials_kernel, dim3(nblocks), dim3(256), 0, s,
                     (const short*)x, numel / 8, (uint32_t*)partials);
  hipLaunchKernelGGL(fp8_scale_final_kernel, dim3(1), dim3(256), 0, s,
                     (const uint32_t*)partials, nblocks, scales);
}

void fp8_cast_transpose_launch(const void* x, const float* scale, void* q,
                               void* qt, int R, int C, hipStream_t s) {
  if (R < 1 || C < 1 || (!q && !qt)) return;
  const int tiles_c = (C + FP8_TILE - 1) / FP8_TILE;
  const int tiles_r = (R + FP8_TILE - 1) / FP8_TILE;
  const dim3 grid((unsigned)((int64_t)tiles_r * tiles_c));
  const short* xs = (const short*)x;
  uint8_t* q8 = (uint8_t*)q;
  uint8_t* qt8 = (uint8_t*)qt;
  if (q && qt)
    hipLaunchKernelGGL((fp8_cast_transpose_kernel<true, true>), grid, dim3(64),
                       0, s, xs, scale, q8, qt8, R, C, tiles_c);
  else if (q)
    hipLaunchKernelGGL((fp8_cast_transpose_kernel<true, false>), grid,
                       dim3(64), 0, s, xs, scale, q8, qt8, R, C, tiles_c);
  else
    hipLaunchKernelGGL((fp8_cast_transpose_kernel<false, true>), grid,
                       dim3(64), 0, s, xs, scale, q8, qt8, R, C, tiles_c);
}
}
