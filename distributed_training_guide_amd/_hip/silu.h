// SwiGLU's forward arithmetic, one copy for every kernel that produces
// h = silu(g) * u (silu_mul.hip, fp8_delayed.hip): f32, the products taken
// left to right.  The callers round the result once to bf16 with f2bf.
#pragma once
#include "common.h"

__device__ __forceinline__ float silu_mul_f32(float g, float u) {
  const float sig = 1.0f / (1.0f + __expf(-g));
  return g * sig * u;
}
