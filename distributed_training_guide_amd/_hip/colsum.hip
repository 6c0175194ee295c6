// Column sum of f32 partials for gfx950: partial [nblocks, H] -> out [H] bf16.
//
// The norm backward kernels (norm.hip) leave one row of
// weight/bias-gradient partials per block; this finishes the reduction.
// Two stages so the read of the (up to 2048 x H) buffer parallelizes over
// enough blocks to reach memory bandwidth (a single H/256-block pass is
// CU-bound): stage 1 folds rows into COLSUM_RY rows, stage 2 finishes.
// No atomics and a fixed fold order: results are run-to-run identical.
#include "common.h"
#include "launchers.h"

__global__ void __launch_bounds__(256) colsum_stage1_kernel(
    const float* __restrict__ partial, float* __restrict__ stage,
    int nblocks, int H) {
  const int y = blockIdx.y;
  const int r0 = (int)(((int64_t)nblocks * y) / COLSUM_RY);
  const int r1 = (int)(((int64_t)nblocks * (y + 1)) / COLSUM_RY);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H;
       i += gridDim.x * blockDim.x) {
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int b = r0;
    for (; b + 8 <= r1; b += 8)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        s[j] += partial[(int64_t)(b + j) * H + i];
    for (; b < r1; ++b) s[0] += partial[(int64_t)b * H + i];
    stage[(int64_t)y * H + i] = ((s[0] + s[1]) + (s[2] + s[3])) +
                                ((s[4] + s[5]) + (s[6] + s[7]));
  }
}

__global__ void __launch_bounds__(256) colsum_stage2_kernel(
    const float* __restrict__ stage, short* __restrict__ out, int H) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H;
       i += gridDim.x * blockDim.x) {
    float s = 0.f;
#pragma unroll
    for (int y = 0; y < COLSUM_RY; ++y) s += stage[(int64_t)y * H + i];
    out[i] = f2bf(s);
  }
}

extern "C" void colsum_launch(float* partial, void* out, int nblocks, int H,
                              hipStream_t s) {
  float* stage = partial + (size_t)nblocks * H;  // the buffer's tail rows
  int rgrid = (H + 255) / 256;
  hipLaunchKernelGGL(colsum_stage1_kernel, dim3(rgrid, COLSUM_RY), dim3(256),
                     0, s, partial, stage, nblocks, H);
  hipLaunchKernelGGL(colsum_stage2_kernel, dim3(rgrid), dim3(256), 0, s,
                     stage, (short*)out, H);
}
