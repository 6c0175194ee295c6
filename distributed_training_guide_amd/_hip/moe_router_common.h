// What the router kernels of moe_router.hip and moe_router_aux.hip share:
// the block shape, the lane-group butterflies, the stable-sort comparison
// and the per-lane logit load.  The mapping they serve is described at the
// top of moe_router.hip.
#pragma once
#include "common.h"

constexpr int MR_WAVES = 4;
constexpr int MR_GRID_CAP = 2048;

template <int LPT>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LPT / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

template <int LPT>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = LPT / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

// (v, i) beats (ov, oi) in a stable descending sort
__device__ __forceinline__ bool mr_better(float v, int i, float ov, int oi) {
  return v > ov || (v == ov && i < oi);
}

// The lane's VPL logits of token t (row-major [T, E]) widened to f32; x1 is
// unused when VPL == 1.
template <int E, int VPL>
__device__ __forceinline__ void mr_load(const short* __restrict__ logits,
                                        int64_t t, int e0, float& x0,
                                        float& x1) {
  if constexpr (VPL == 2) {
    const uint32_t u =
        *reinterpret_cast<const uint32_t*>(logits + t * E + e0);
    x0 = bf2f((short)(u & 0xffffu));
    x1 = bf2f((short)(u >> 16));
  } else {
    x0 = bf2f(logits[t * E + e0]);
    x1 = -INFINITY;
  }
}

// One block per MR_WAVES * (tokens per wave) tokens up to `cap`, past which
// the kernels grid-stride; never an empty grid (host side).
inline int mr_grid(int64_t T, int E, int cap) {
  const int tpw = E < WAVE ? WAVE / E : 1;
  const int64_t per_block = (int64_t)MR_WAVES * tpw;
  const int64_t want = (T + per_block - 1) / per_block;
  return (int)(want < 1 ? 1 : want < cap ? want : cap);
}

// Launch KERNEL<E, NORM> for the run-time E and `norm` in scope on `grid`
// blocks of 256 threads of stream `s`.
#define MR_DISPATCH(KERNEL, grid, ...)                                      \
  do {                                                                      \
    const dim3 block(256);                                                  \
    switch (E * 2 + (norm ? 1 : 0)) {                                       \
      case 17: hipLaunchKernelGGL((KERNEL<8, true>), grid, block, 0, s, __VA_ARGS__); break;    \
      case 16: hipLaunchKernelGGL((KERNEL<8, false>), grid, block, 0, s, __VA_ARGS__); break;   \
      case 33: hipLaunchKernelGGL((KERNEL<16, true>), grid, block, 0, s, __VA_ARGS__); break;   \
      case 32: hipLaunchKernelGGL((KERNEL<16, false>), grid, block, 0, s, __VA_ARGS__); break;  \
      case 65: hipLaunchKernelGGL((KERNEL<32, true>), grid, block, 0, s, __VA_ARGS__); break;   \
      case 64: hipLaunchKernelGGL((KERNEL<32, false>), grid, block, 0, s, __VA_ARGS__); break;  \
      case 129: hipLaunchKernelGGL((KERNEL<64, true>), grid, block, 0, s, __VA_ARGS__); break;  \
      case 128: hipLaunchKernelGGL((KERNEL<64, false>), grid, block, 0, s, __VA_ARGS__); break; \
      case 257: hipLaunchKernelGGL((KERNEL<128, true>), grid, block, 0, s, __VA_ARGS__); break; \
      case 256: hipLaunchKernelGGL((KERNEL<128, false>), grid, block, 0, s, __VA_ARGS__); break;\
      default: break; /* the binding rejects every other E */               \
    }                                                                       \
  } while (0)
