// Embedding gather (fwd) + scatter-add (bwd) for gfx950 — the token
// lookup the reference gets from torch's nn.Embedding (SURVEY.md §2b
// "Embedding gather + LM-head GEMM"; VERDICT round-1 flagged the torch op
// as the one non-native hot-loop kernel).
//
// fwd: out[r, :] = table[ids[r], :] — one wave per row, bf16x8 loads.
// bwd: dtable[id, :] += dy[r, :] with collisions — accumulate into an
//      fp32 workspace with atomicAdd (frequent tokens collide; bf16
//      packed atomics would round-to-nearest per add and bias heavy
//      hitters), then convert once to the bf16 grad.
#include "common.h"
#include "launchers.h"

__global__ void __launch_bounds__(256) embed_fwd_kernel(
    const short* __restrict__ table, const int64_t* __restrict__ ids,
    short* __restrict__ out, int64_t nrows, int H, int64_t V) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int waves = blockDim.x / WAVE;
  for (int64_t r = (int64_t)blockIdx.x * waves + wave; r < nrows;
       r += (int64_t)gridDim.x * waves) {
    int64_t id = ids[r];
    DTGA_KERNEL_ASSERT(id >= 0 && id < V);
    const short* src = table + id * H;
    short* dst = out + r * H;
    if ((H & 7) == 0) {
      for (int i = lane * 8; i < H; i += WAVE * 8)
        *reinterpret_cast<s16x8*>(dst + i) =
            *reinterpret_cast<const s16x8*>(src + i);
    } else {
      for (int i = lane; i < H; i += WAVE) dst[i] = src[i];
    }
  }
}

__global__ void __launch_bounds__(256) embed_bwd_scatter_kernel(
    const short* __restrict__ dy, const int64_t* __restrict__ ids,
    float* __restrict__ acc, int64_t nrows, int H, int64_t V) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int waves = blockDim.x / WAVE;
  for (int64_t r = (int64_t)blockIdx.x * waves + wave; r < nrows;
       r += (int64_t)gridDim.x * waves) {
    int64_t id = ids[r];
    DTGA_KERNEL_ASSERT(id >= 0 && id < V);
    const short* src = dy + r * H;
    float* dst = acc + id * H;
    if ((H & 3) == 0) {
      for (int i = lane * 4; i < H; i += WAVE * 4) {
        s16x4 v = *reinterpret_cast<const s16x4*>(src + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(dst + i + j, bf2f(v[j]));
      }
    } else {
      for (int i = lane; i < H; i += WAVE) atomicAdd(dst + i, bf2f(src[i]));
    }
  }
}

__global__ void __launch_bounds__(256) f32_to_bf16_kernel(
    const float* __restrict__ src, short* __restrict__ dst, int64_t n) {
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
       i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
    if (i + 4 <= n) {
      f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
      s16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = f2bf(v[j]);
      *reinterpret_cast<s16x4*>(dst + i) = o;
    } else {
      for (int64_t j = i; j < n; ++j) dst[j] = f2bf(src[j]);
    }
  }
}

extern "C" {
void embed_fwd_launch(const void* table, const int64_t* ids, void* out,
                      int64_t nrows, int H, int64_t V, hipStream_t s) {
  int waves = 4;
  int64_t blocks = (nrows + waves - 1) / waves;
  int grid = (int)(blocks < 8192 ? (blocks < 1 ? 1 : blocks) : 8192);
  hipLaunchKernelGGL(embed_fwd_kernel, dim3(grid), dim3(256), 0, s,
                     (const short*)table, ids, (short*)out, nrows, H, V);
}
void embed_bwd_launch(const void* dy, const int64_t* ids, float* acc,
                      void* dtable, int64_t nrows, int H, int64_t V,
                      hipStream_t s) {
  hipMemsetAsync(acc, 0, (size_t)V * H * sizeof(float), s);
  int waves = 4;
  int64_t blocks = (nrows + waves - 1) / waves;
  int grid = (int)(blocks < 8192 ? (blocks < 1 ? 1 : blocks) : 8192);
  hipLaunchKernelGGL(embed_bwd_scatter_kernel, dim3(grid), dim3(256), 0, s,
                     (const short*)dy, ids, acc, nrows, H, V);
  int64_t n = V * (int64_t)H;
  int64_t cblocks = (n / 4 + 255) / 256;
  // never an empty grid: V*H < 4 is all tail
  int cgrid = (int)(cblocks < 1 ? 1 : cblocks < 8192 ? cblocks : 8192);
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(cgrid), dim3(256), 0, s,
                     acc, (short*)dtable, n);
}
}
