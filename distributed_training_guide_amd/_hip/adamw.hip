// Fused multi-tensor AdamW for gfx950 (SURVEY.md §2b "Fused AdamW";
// reference uses torch.optim.AdamW(fused=True) at 01:73, 02:88, 04:113,
// 05:197, 06:151, 07:152).
//
// One launch updates every parameter chunk: the host packs chunk descriptors
// (pointers + length + dtypes) into an int64 device tensor, one 256-thread
// block per chunk, grid-stride within the chunk. Moments are fp32; params
// bf16 or fp32; grads bf16 or fp32 (fp32 under FSDP's reduce_dtype=fp32).
// Decoupled weight decay (AdamW): p *= (1 - lr*wd) before the Adam update.
#include "common.h"
#include "launchers.h"

#define ADAMW_CHUNK 262144  // elements per descriptor chunk

// AdamWDesc (the chunk descriptor) lives in common.h, shared with
// grad_norm.hip.

typedef __attribute__((ext_vector_type(4))) short s16x4v;

// ---- 16-bit-extended master weights (MASTER instantiations) ----
// A bf16 parameter `hi` and an int16 companion `lo` (state["master_lo"])
// together hold an fp32 master exactly.  For the master's bit pattern u, in
// 32-bit wrap-around arithmetic:
//   hi = (u + 0x8000) >> 16      lo = int16(u - (hi << 16))
//   u  = (hi << 16) + sext(lo)
// hi is u rounded to nearest on the magnitude, ties AWAY from zero (not
// f2bf's ties-to-even: that remainder would need +-0x8000, which does not
// fit 16 bits), so lo always lies in [-32768, 32767].  A NaN master is
// stored as (0x7FC0, 0): the wrapped hi of a NaN can be +-0 or +-inf, and
// the forward pass, which reads hi alone, must see a NaN.  A finite master
// above the largest bf16 shows as bf16 inf while the pair stays finite.
// ops/adamw.py split_master / join_master are the same rule on the host.
__device__ __forceinline__ float master_join(short hi, short lo) {
  const uint32_t u = (((uint32_t)(uint16_t)hi) << 16) + (uint32_t)(int32_t)lo;
  return __builtin_bit_cast(float, u);
}

__device__ __forceinline__ void master_split(float f, short& hi, short& lo) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  uint32_t h = (u + 0x8000u) >> 16;
  uint32_t l = u - (h << 16);
  if ((u & 0x7fffffffu) > 0x7f800000u) {  // NaN
    h = 0x7fc0u;
    l = 0u;
  }
  hi = (short)h;
  lo = (short)l;
}

// The per-element update, written once: every instantiation and both the
// vector body and the scalar tail call it, so a master-weight bf16 parameter
// rounds exactly like an fp32 parameter.
__device__ __forceinline__ void adamw_update(float g, float& m, float& v,
                                             float& p, float lr, float beta1,
                                             float beta2, float eps,
                                             float decay, float inv_bc1,
                                             float inv_bc2) {
  m = beta1 * m + (1.0f - beta1) * g;
  v = beta2 * v + (1.0f - beta2) * g * g;
  p = p * decay - lr * (m * inv_bc1) / (sqrtf(v * inv_bc2) + eps);
}

// CLIP=true is global-norm gradient clipping fused into the update: the
// scale comes from the device-resident total squared grad sum (written by
// grad_norm.hip) and multiplies g right after the load, before the moment
// updates — grads are never rewritten and the host never waits.  CLIP=false
// is the unclipped arithmetic, unchanged.
// MASTER=true: lo_tab[c] is chunk c's int16 companion (0 for an fp32
// parameter, which takes the plain path and has none).  A bf16 chunk loads
// p and lo, rebuilds the fp32 master, updates it and stores both halves,
// 16 B each per 8 elements: 26 B of traffic per element for 22.
template <bool CLIP, bool MASTER>
__global__ void __launch_bounds__(256) adamw_kernel(
    const AdamWDesc* __restrict__ descs, int nchunks, float lr, float beta1,
    float beta2, float eps, float wd, float inv_bc1, float inv_bc2,
    const float* __restrict__ sq_total, float max_norm,
    const int64_t* __restrict__ lo_tab) {
  float coef = 1.0f;
  if constexpr (CLIP) coef = clip_coef(sq_total, max_norm);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    AdamWDesc d = descs[c];
    float* m = (float*)d.m;
    float* v = (float*)d.v;
    short* lo = nullptr;
    if constexpr (MASTER) lo = (short*)lo_tab[c];
    const bool pbf = d.p_is_bf16 != 0;
    const bool gbf = d.g_is_bf16 != 0;
    const float decay = 1.0f - lr * wd;
    // vectorized main body: 8 elements per thread per iteration (2x 16 B
    // f32 moment streams in flight — memory-bound, G13 vectorization +
    // deeper MLP; update via rsqrt: p -= lr*m̂ * rsqrt-style reciprocal)
    const int64_t n8 = d.n / 8;
    for (int64_t qq = threadIdx.x; qq < n8; qq += blockDim.x) {
      int64_t i = qq * 8;
      f32x4 g4[2], p4[2], m4[2], v4[2];
      if (gbf) {
        s16x8 gv = *reinterpret_cast<const s16x8*>((const short*)d.g + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) g4[j >> 2][j & 3] = bf2f(gv[j]);
      } else {
        g4[0] = *reinterpret_cast<const f32x4*>((const float*)d.g + i);
        g4[1] = *reinterpret_cast<const f32x4*>((const float*)d.g + i + 4);
      }
      if constexpr (CLIP) {
        g4[0] *= coef;
        g4[1] *= coef;
      }
      if (pbf) {
        s16x8 pv = *reinterpret_cast<const s16x8*>((const short*)d.p + i);
        if constexpr (MASTER) {
          s16x8 lv = *reinterpret_cast<const s16x8*>(lo + i);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            p4[j >> 2][j & 3] = master_join(pv[j], lv[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) p4[j >> 2][j & 3] = bf2f(pv[j]);
        }
      } else {
        p4[0] = *reinterpret_cast<const f32x4*>((const float*)d.p + i);
        p4[1] = *reinterpret_cast<const f32x4*>((const float*)d.p + i + 4);
      }
      m4[0] = *reinterpret_cast<const f32x4*>(m + i);
      m4[1] = *reinterpret_cast<const f32x4*>(m + i + 4);
      v4[0] = *reinterpret_cast<const f32x4*>(v + i);
      v4[1] = *reinterpret_cast<const f32x4*>(v + i + 4);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float mi = m4[h][j], vi = v4[h][j], pi = p4[h][j];
          adamw_update(g4[h][j], mi, vi, pi, lr, beta1, beta2, eps, decay,
                       inv_bc1, inv_bc2);
          m4[h][j] = mi;
          v4[h][j] = vi;
          p4[h][j] = pi;
        }
      *reinterpret_cast<f32x4*>(m + i) = m4[0];
      *reinterpret_cast<f32x4*>(m + i + 4) = m4[1];
      *reinterpret_cast<f32x4*>(v + i) = v4[0];
      *reinterpret_cast<f32x4*>(v + i + 4) = v4[1];
      if (pbf) {
        s16x8 pv;
        if constexpr (MASTER) {
          s16x8 lv;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            short hj, lj;
            master_split(p4[j >> 2][j & 3], hj, lj);
            pv[j] = hj;
            lv[j] = lj;
          }
          *reinterpret_cast<s16x8*>(lo + i) = lv;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) pv[j] = f2bf(p4[j >> 2][j & 3]);
        }
        *reinterpret_cast<s16x8*>((short*)d.p + i) = pv;
      } else {
        *reinterpret_cast<f32x4*>((float*)d.p + i) = p4[0];
        *reinterpret_cast<f32x4*>((float*)d.p + i + 4) = p4[1];
      }
    }
    // scalar tail
    for (int64_t i = n8 * 8 + threadIdx.x; i < d.n; i += blockDim.x) {
      float g = gbf ? bf2f(((const short*)d.g)[i]) : ((const float*)d.g)[i];
      if constexpr (CLIP) g *= coef;
      float p;
      if (!pbf) p = ((const float*)d.p)[i];
      else if constexpr (MASTER) p = master_join(((const short*)d.p)[i], lo[i]);
      else p = bf2f(((const short*)d.p)[i]);
      float mi = m[i], vi = v[i];
      adamw_update(g, mi, vi, p, lr, beta1, beta2, eps, decay, inv_bc1,
                   inv_bc2);
      m[i] = mi;
      v[i] = vi;
      if (!pbf) {
        ((float*)d.p)[i] = p;
      } else if constexpr (MASTER) {
        short hj, lj;
        master_split(p, hj, lj);
        ((short*)d.p)[i] = hj;
        lo[i] = lj;
      } else {
        ((short*)d.p)[i] = f2bf(p);
      }
    }
  }
}

template <bool CLIP, bool MASTER>
static void adamw_launch_impl(const void* descs, const int64_t* lo_tab,
                              int nchunks, float lr, float beta1, float beta2,
                              float eps, float wd, float inv_bc1,
                              float inv_bc2, const float* sq_total,
                              float max_norm, hipStream_t s) {
  int grid = nchunks < 16384 ? nchunks : 16384;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((adamw_kernel<CLIP, MASTER>), dim3(grid), dim3(256), 0,
                     s, (const AdamWDesc*)descs, nchunks, lr, beta1, beta2,
                     eps, wd, inv_bc1, inv_bc2, sq_total, max_norm, lo_tab);
}

extern "C" {
void adamw_launch(const void* descs, int nchunks, float lr, float beta1,
                  float beta2, float eps, float wd, float inv_bc1,
                  float inv_bc2, hipStream_t s) {
  adamw_launch_impl<false, false>(descs, nullptr, nchunks, lr, beta1, beta2,
                                  eps, wd, inv_bc1, inv_bc2, nullptr, 0.0f, s);
}

void adamw_launch_clipped(const void* descs, int nchunks, float lr,
                          float beta1, float beta2, float eps, float wd,
                          float inv_bc1, float inv_bc2, const float* sq_total,
                          float max_norm, hipStream_t s) {
  adamw_launch_impl<true, false>(descs, nullptr, nchunks, lr, beta1, beta2,
                                 eps, wd, inv_bc1, inv_bc2, sq_total,
                                 max_norm, s);
}

void adamw_master_launch(const void* descs, const int64_t* lo_tab,
                         int nchunks, float lr, float beta1, float beta2,
                         float eps, float wd, float inv_bc1, float inv_bc2,
                         const float* sq_total, float max_norm,
                         hipStream_t s) {
  if (sq_total)
    adamw_launch_impl<true, true>(descs, lo_tab, nchunks, lr, beta1, beta2,
                                  eps, wd, inv_bc1, inv_bc2, sq_total,
                                  max_norm, s);
  else
    adamw_launch_impl<false, true>(descs, lo_tab, nchunks, lr, beta1, beta2,
                                   eps, wd, inv_bc1, inv_bc2, nullptr, 0.0f,
                                   s);
}
}
