// tanh-GELU forward/backward for gfx950 — the GPT-2 MLP activation
// (reference chapter-1 smoke model trains HF gpt2, whose GELU comes from
// transformers; SURVEY.md §2b "torch.compile fusions").  Elementwise,
// bf16x8 vector loads, f32 arithmetic.
//
//   gelu(x) = 0.5 x (1 + tanh(k (x + 0.044715 x^3))), k = sqrt(2/pi)
#include "common.h"
#include "launchers.h"

#define GELU_K 0.7978845608028654f
#define GELU_C 0.044715f

// ---------------- tanh-GELU ----------------
__global__ void __launch_bounds__(256) gelu_fwd_kernel(
    const short* __restrict__ x, short* __restrict__ y, int64_t n) {
  for (int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
       idx < n; idx += (int64_t)gridDim.x * blockDim.x * 8) {
    s16x8 v = *reinterpret_cast<const s16x8*>(x + idx);
    s16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(v[j]);
      float t = tanhf(GELU_K * (f + GELU_C * f * f * f));
      o[j] = f2bf(0.5f * f * (1.0f + t));
    }
    *reinterpret_cast<s16x8*>(y + idx) = o;
  }
}

__global__ void __launch_bounds__(256) gelu_bwd_kernel(
    const short* __restrict__ dy, const short* __restrict__ x,
    short* __restrict__ dx, int64_t n) {
  for (int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
       idx < n; idx += (int64_t)gridDim.x * blockDim.x * 8) {
    s16x8 dv = *reinterpret_cast<const s16x8*>(dy + idx);
    s16x8 v = *reinterpret_cast<const s16x8*>(x + idx);
    s16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(v[j]);
      float t = tanhf(GELU_K * (f + GELU_C * f * f * f));
      float du = GELU_K * (1.0f + 3.0f * GELU_C * f * f);
      float d = 0.5f * (1.0f + t) + 0.5f * f * (1.0f - t * t) * du;
      o[j] = f2bf(bf2f(dv[j]) * d);
    }
    *reinterpret_cast<s16x8*>(dx + idx) = o;
  }
}

extern "C" {
void gelu_fwd_launch(const void* x, void* y, int64_t n, hipStream_t s) {
  int64_t blocks = (n / 8 + 255) / 256;
  int grid = (int)(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096);
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(grid), dim3(256), 0, s,
                     (const short*)x, (short*)y, n);
}

void gelu_bwd_launch(const void* dy, const void* x, void* dx, int64_t n,
                     hipStream_t s) {
  int64_t blocks = (n / 8 + 255) / 256;
  int grid = (int)(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096);
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(grid), dim3(256), 0, s,
                     (const short*)dy, (const short*)x, (short*)dx, n);
}
}
