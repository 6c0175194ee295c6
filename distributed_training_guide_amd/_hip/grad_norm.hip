// Multi-tensor global gradient norm for gfx950: the read-only pass behind
// fused gradient clipping (ops/grad_clip.py, FusedAdamW(max_grad_norm=...)).
//
// Same chunk-descriptor table as adamw.hip (AdamWDesc in common.h; only g,
// n and g_is_bf16 are read), one 256-thread block per chunk, grid-striding
// over chunks.  grad_sqsum writes one fp32 partial per chunk with an
// ordinary store and a second single-block kernel folds the partials in a
// fixed order — no atomics, so the result is bitwise reproducible and no
// buffer needs pre-zeroing.  The total stays on the device: grad_scale and
// the clipped AdamW kernel read it through a pointer, the host never waits.
//
// Unlike adamw.hip, a chunk base that is only element-aligned (a view into
// a DDP bucket, buf[1:]) is supported: a scalar head is peeled up to the
// next 16 B boundary before the 8-element vector body.
#include "common.h"
#include "launchers.h"

// elements to peel so that (base + head) is 16 B aligned (base is
// element-aligned), clamped to the chunk length
__device__ __forceinline__ int64_t align_head(int64_t base, int esz,
                                              int64_t n) {
  const int64_t head = ((16 - (base & 15)) & 15) / esz;
  return head < n ? head : n;
}

__global__ void __launch_bounds__(256) grad_sqsum_partials_kernel(
    const AdamWDesc* __restrict__ descs, int nchunks,
    float* __restrict__ partials) {
  __shared__ float scratch[4];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    AdamWDesc d = descs[c];
    const bool gbf = d.g_is_bf16 != 0;
    const int64_t head = align_head(d.g, gbf ? 2 : 4, d.n);
    const int64_t n8 = (d.n - head) / 8;
    // two independent accumulators per thread: the fp32 add chain is at
    // most 4 * ceil(n8 / 256) long (512 for a full 262144-element chunk)
    float acc0 = 0.0f, acc1 = 0.0f;
    if (gbf) {
      const short* g = (const short*)d.g;
      if (threadIdx.x < head) {
        float x = bf2f(g[threadIdx.x]);
        acc0 += x * x;
      }
      const short* gb = g + head;
#pragma unroll 4
      for (int64_t qq = threadIdx.x; qq < n8; qq += blockDim.x) {
        s16x8 gv = *reinterpret_cast<const s16x8*>(gb + qq * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = bf2f(gv[j]), b = bf2f(gv[4 + j]);
          acc0 += a * a;
          acc1 += b * b;
        }
      }
      for (int64_t i = head + n8 * 8 + threadIdx.x; i < d.n; i += blockDim.x) {
        float x = bf2f(g[i]);
        acc1 += x * x;
      }
    } else {
      const float* g = (const float*)d.g;
      if (threadIdx.x < head) {
        float x = g[threadIdx.x];
        acc0 += x * x;
      }
      const float* gb = g + head;
#pragma unroll 4
      for (int64_t qq = threadIdx.x; qq < n8; qq += blockDim.x) {
        f32x4 a = *reinterpret_cast<const f32x4*>(gb + qq * 8);
        f32x4 b = *reinterpret_cast<const f32x4*>(gb + qq * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc0 += a[j] * a[j];
          acc1 += b[j] * b[j];
        }
      }
      for (int64_t i = head + n8 * 8 + threadIdx.x; i < d.n; i += blockDim.x) {
        float x = g[i];
        acc1 += x * x;
      }
    }
    const float total = block_reduce_sum(acc0 + acc1, scratch);
    if (threadIdx.x == 0) partials[c] = total;
  }
}

// <<<1, 256>>>: fold partials[0..nchunks) into out[slot].  Each thread
// strides over the partials in double, then a fixed-order LDS tree.
__global__ void __launch_bounds__(256) grad_sqsum_final_kernel(
    const float* __restrict__ partials, int nchunks, float* __restrict__ out,
    int slot) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nchunks; i += 256) acc += (double)partials[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[slot] = (float)sh[0];
}

// g *= coef in place over the same table; coef is computed in-kernel from
// the device-resident total.  coef == 1 (norm within max_norm) leaves the
// grads untouched without the read-modify-write pass.
__global__ void __launch_bounds__(256) grad_scale_kernel(
    const AdamWDesc* __restrict__ descs, int nchunks,
    const float* __restrict__ sq_total, float max_norm) {
  const float coef = clip_coef(sq_total, max_norm);
  if (coef == 1.0f) return;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    AdamWDesc d = descs[c];
    const bool gbf = d.g_is_bf16 != 0;
    const int64_t head = align_head(d.g, gbf ? 2 : 4, d.n);
    const int64_t n8 = (d.n - head) / 8;
    if (gbf) {
      short* g = (short*)d.g;
      if (threadIdx.x < head) g[threadIdx.x] = f2bf(bf2f(g[threadIdx.x]) * coef);
      short* gb = g + head;
      for (int64_t qq = threadIdx.x; qq < n8; qq += blockDim.x) {
        s16x8 gv = *reinterpret_cast<const s16x8*>(gb + qq * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] = f2bf(bf2f(gv[j]) * coef);
        *reinterpret_cast<s16x8*>(gb + qq * 8) = gv;
      }
      for (int64_t i = head + n8 * 8 + threadIdx.x; i < d.n; i += blockDim.x)
        g[i] = f2bf(bf2f(g[i]) * coef);
    } else {
      float* g = (float*)d.g;
      if (threadIdx.x < head) g[threadIdx.x] *= coef;
      float* gb = g + head;
      for (int64_t qq = threadIdx.x; qq < n8; qq += blockDim.x) {
        f32x4 a = *reinterpret_cast<const f32x4*>(gb + qq * 8);
        f32x4 b = *reinterpret_cast<const f32x4*>(gb + qq * 8 + 4);
        *reinterpret_cast<f32x4*>(gb + qq * 8) = a * coef;
        *reinterpret_cast<f32x4*>(gb + qq * 8 + 4) = b * coef;
      }
      for (int64_t i = head + n8 * 8 + threadIdx.x; i < d.n; i += blockDim.x)
        g[i] *= coef;
    }
  }
}

extern "C" {
void grad_sqsum_launch(const void* descs, int nchunks, float* partials,
                       float* out, int slot, hipStream_t s) {
  if (nchunks > 0) {
    const int grid = nchunks < 16384 ? nchunks : 16384;
    hipLaunchKernelGGL(grad_sqsum_partials_kernel, dim3(grid), dim3(256), 0,
                       s, (const AdamWDesc*)descs, nchunks, partials);
  }
  hipLaunchKernelGGL(grad_sqsum_final_kernel, dim3(1), dim3(256), 0, s,
                     (const float*)partials, nchunks, out, slot);
}

void grad_scale_launch(const void* descs, int nchunks, const float* sq_total,
                       float max_norm, hipStream_t s) {
  if (nchunks < 1) return;
  const int grid = nchunks < 16384 ? nchunks : 16384;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(grid), dim3(256), 0, s,
                     (const AdamWDesc*)descs, nchunks, sq_total, max_norm);
}
}
