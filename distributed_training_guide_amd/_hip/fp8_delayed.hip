// Delayed-scaling e4m3 quantisation for gfx950 (ops/fp8_linear.py,
// recipe="delayed").  The scale is known before the tensor is read (it comes
// from the amaxes of earlier steps), so one pass over the tensor casts it and
// takes this step's amax as a by-product, and a producer can write e4m3
// directly.  Three kernels, all on the 64x64 tile of fp8_tile.h (one wave per
// tile, a 4x16 bf16 patch per lane, the row-major copy from registers, the
// transposed copy through the swizzled 4 KiB LDS image):
//
//   fp8_cast_amax_kernel<ROW, TR>: fp8_cast_transpose_kernel plus the amax.
//     The lane already holds its 64 raw bf16 values: integer max of their
//     sign-cleared bits (exact, a NaN wins), a wave butterfly, one ordinary
//     store of the tile's partial.  No atomics, no pre-zeroed buffer: a lane
//     outside the tensor contributes 0 and every tile stores.
//     4 B per element with both outputs against the two-pass 6 B.
//
//   silu_mul_fp8_kernel: the same tile, but the patch is h = silu(g) * u of
//     the packed gate|up row [R, 2I]: sixteen 16 B loads, silu_mul_f32 of
//     silu.h (the function silu_mul.hip calls), one rounding to bf16 in
//     registers exactly where silu_mul rounds.  From there the patch is
//     indistinguishable from one loaded from a bf16 h, so bytes and amax
//     equal the unfused chain's bit for bit, and h never exists in memory:
//     6 B per element of h against 12 B.
//
//   fp8_history_update_kernel <<<1, 1024>>>: folds the tile partials (16 B
//     loads, about 21 independent loads a thread for the 86 016 tiles of a
//     [24576, 14336] tensor, so one block is enough), writes the amax into the
//     history slot and the scale pair of max(history) into a fresh [2]
//     buffer with the two IEEE divisions and the compare floor of
//     fp8_scale_final_kernel.  slot < 0 seeds: every slot gets the amax.
//     A non-finite amax does not enter the history: the slot gets the
//     previous max(history) instead, so one bad step does not poison the next
//     L (its own output is NaN wherever the input was: the cast hides
//     nothing).  A history that is itself non-finite (seeded by a non-finite
//     tensor) is re-seeded by the first finite amax.
#include "common.h"
#include "fp8_tile.h"
#include "launchers.h"
#include "silu.h"

template <bool ROW, bool TR>
__global__ void __launch_bounds__(64) fp8_cast_amax_kernel(
    const short* __restrict__ x, const float* __restrict__ scale_p,
    uint8_t* __restrict__ q, uint8_t* __restrict__ qt,
    uint32_t* __restrict__ partials, int R, int C, int tiles_c) {
  __shared__ __attribute__((aligned(16))) uint32_t image[FP8_TILE * 16];
  const Fp8Tile t = fp8_tile(R, C, tiles_c);
  uint32_t m = 0;
  if (t.inside) {
    const float scale = *scale_p;
    s16x8 raw[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const short* src = x + (int64_t)(t.r0 + i) * C + t.c0;
      raw[i][0] = *reinterpret_cast<const s16x8*>(src);
      raw[i][1] = *reinterpret_cast<const s16x8*>(src + 8);
    }
    m = fp8_patch_umax(raw);
    fp8_patch_store<ROW, TR>(raw, scale, t, image, q, C);
  }
  if constexpr (TR) fp8_image_flush(image, t, qt, R, C);
  m = wave_reduce_umax(m);
  if (t.lane == 0) partials[blockIdx.x] = m;
}

// gu [R, 2I] = gate | up; q [R, I], qt [I, R]
__global__ void __launch_bounds__(64) silu_mul_fp8_kernel(
    const short* __restrict__ gu, const float* __restrict__ scale_p,
    uint8_t* __restrict__ q, uint8_t* __restrict__ qt,
    uint32_t* __restrict__ partials, int R, int I, int tiles_c) {
  __shared__ __attribute__((aligned(16))) uint32_t image[FP8_TILE * 16];
  const Fp8Tile t = fp8_tile(R, I, tiles_c);
  uint32_t m = 0;
  if (t.inside) {
    const float scale = *scale_p;
    s16x8 raw[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const short* g = gu + (int64_t)(t.r0 + i) * (2 * (int64_t)I) + t.c0;
      const short* u = g + I;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const s16x8 gv = *reinterpret_cast<const s16x8*>(g + 8 * h);
        const s16x8 uv = *reinterpret_cast<const s16x8*>(u + 8 * h);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          raw[i][h][j] = f2bf(silu_mul_f32(bf2f(gv[j]), bf2f(uv[j])));
      }
    }
    m = fp8_patch_umax(raw);
    fp8_patch_store<true, true>(raw, scale, t, image, q, I);
  }
  fp8_image_flush(image, t, qt, R, I);
  m = wave_reduce_umax(m);
  if (t.lane == 0) partials[blockIdx.x] = m;
}

__global__ void __launch_bounds__(1024) fp8_history_update_kernel(
    const uint32_t* __restrict__ partials, int nparts,
    float* __restrict__ history, int L, int slot, float* __restrict__ out) {
  __shared__ uint32_t sh[16];
  const int tid = threadIdx.x;
  uint32_t m = 0;
  const int n4 = nparts >> 2;
  for (int i = tid; i < n4; i += 1024) {
    const u32x4 v = reinterpret_cast<const u32x4*>(partials)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) m = v[j] > m ? v[j] : m;
  }
  for (int i = (n4 << 2) + tid; i < nparts; i += 1024) {
    const uint32_t p = partials[i];
    m = p > m ? p : m;
  }
  m = wave_reduce_umax(m);
  if ((tid & (WAVE - 1)) == 0) sh[tid >> 6] = m;
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < 16; ++w) m = sh[w] > m ? sh[w] : m;

  const bool finite = m < 0x7f80u;
  const float amax = bf2f((short)m);
  // a NaN in the history is in every slot (see below), so slot 0 keeps it
  float prev = history[0];
  for (int i = 1; i < L; ++i) prev = history[i] > prev ? history[i] : prev;
  float hmax;
  if (slot < 0 || !(prev < INFINITY)) {
    hmax = finite ? amax : __builtin_nanf("");
    for (int i = 0; i < L; ++i) history[i] = hmax;
  } else {
    const float v = finite ? amax : prev;
    history[slot] = v;
    hmax = v;
    for (int i = 0; i < L; ++i) hmax = history[i] > hmax ? history[i] : hmax;
  }
  // a compare, not fmaxf: a NaN stays NaN (fp8_scale_final_kernel)
  const float a = hmax < FP8_AMAX_FLOOR ? FP8_AMAX_FLOOR : hmax;
  out[0] = __fdiv_rn(FP8_E4M3_MAX, a);
  out[1] = __fdiv_rn(a, FP8_E4M3_MAX);
}

extern "C" {
int64_t fp8_tiles(int R, int C) {
  return (int64_t)((R + FP8_TILE - 1) / FP8_TILE) *
         ((C + FP8_TILE - 1) / FP8_TILE);
}

void fp8_cast_amax_launch(const void* x, const float* scale, void* q,
                          void* qt, void* partials, int R, int C,
                          hipStream_t s) {
  if (R < 1 || C < 1 || (!q && !qt)) return;
  const int tiles_c = (C + FP8_TILE - 1) / FP8_TILE;
  const dim3 grid((unsigned)fp8_tiles(R, C));
  const short* xs = (const short*)x;
  uint8_t* q8 = (uint8_t*)q;
  uint8_t* qt8 = (uint8_t*)qt;
  uint32_t* pp = (uint32_t*)partials;
  if (q && qt)
    hipLaunchKernelGGL((fp8_cast_amax_kernel<true, true>), grid, dim3(64), 0,
                       s, xs, scale, q8, qt8, pp, R, C, tiles_c);
  else if (q)
    hipLaunchKernelGGL((fp8_cast_amax_kernel<true, false>), grid, dim3(64), 0,
                       s, xs, scale, q8, qt8, pp, R, C, tiles_c);
  else
    hipLaunchKernelGGL((fp8_cast_amax_kernel<false, true>), grid, dim3(64), 0,
                       s, xs, scale, q8, qt8, pp, R, C, tiles_c);
}

void silu_mul_fp8_launch(const void* gu, const float* scale, void* q, void* qt,
                         void* partials, int R, int I, hipStream_t s) {
  if (R < 1 || I < 1) return;
  const int tiles_c = (I + FP8_TILE - 1) / FP8_TILE;
  hipLaunchKernelGGL(silu_mul_fp8_kernel, dim3((unsigned)fp8_tiles(R, I)),
                     dim3(64), 0, s, (const short*)gu, scale, (uint8_t*)q,
                     (uint8_t*)qt, (uint32_t*)partials, R, I, tiles_c);
}

void fp8_history_update_launch(const void* partials, int nparts,
                               float* history, int L, int slot, float* out,
                               hipStream_t s) {
  hipLaunchKernelGGL(fp8_history_update_kernel, dim3(1), dim3(1024), 0, s,
                     (const uint32_t*)partials, nparts, history, L, slot,
                     out);
}
}
