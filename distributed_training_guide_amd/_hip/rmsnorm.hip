// Fused RMSNorm forward/backward for gfx950, plain and with the residual
// add folded in.
//
// Replaces the reference's LlamaRMSNorm (transformers; invoked from every
// Llama forward — see SURVEY.md §2b "RMSNorm"). One workgroup per row,
// bf16x8 vectorized loads (G13), f32 accumulation, wave+block shuffle
// reductions. Forward saves rstd (f32 per row) for the backward.
//
//   y = x * rsqrt(mean(x^2) + eps) * w
//   dx = rstd * (g - xhat * mean(g * xhat)),  g = dy * w,  xhat = x * rstd
//   dw = sum_rows dy * xhat   (per-block partials, then colsum.hip)
//
// The decoder stack threads a (delta, residual) pair between layers:
//   res_out = residual + delta;  y = rmsnorm(res_out) * w
// fused into one pass (read res+delta, write res_out+y) — the unfused
// chain costs an extra full read+write of the hidden state per boundary
// plus the backward's gradient-accumulation elementwise adds.  Its
// backward takes dy = d_normed and dr = d_res_out, x = res_out:
//   dx = rstd * (g - xhat * mean(g * xhat)) + dr      (d_residual = d_delta)
#include "common.h"
#include "launchers.h"

// ---------------- forward ----------------
__global__ void __launch_bounds__(256) rmsnorm_fwd_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    short* __restrict__ y, float* __restrict__ rstd_out,
    int64_t nrows, int H, float eps) {
  __shared__ float scratch[8];
  const float invH = 1.0f / (float)H;
  for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const short* xr = x + row * H;
    short* yr = y + row * H;
    float ss = 0.0f;
    if ((H & 7) == 0) {
      for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        s16x8 v = *reinterpret_cast<const s16x8*>(xr + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) { float f = bf2f(v[j]); ss += f * f; }
      }
    } else {
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        float f = bf2f(xr[i]); ss += f * f;
      }
    }
    ss = block4_sum(ss, scratch);
    const float rstd = rsqrtf(ss * invH + eps);
    if (threadIdx.x == 0 && rstd_out != nullptr) rstd_out[row] = rstd;
    if ((H & 7) == 0) {
      for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        s16x8 v = *reinterpret_cast<const s16x8*>(xr + i);
        s16x8 wv = *reinterpret_cast<const s16x8*>(w + i);
        s16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(v[j]) * rstd * bf2f(wv[j]));
        *reinterpret_cast<s16x8*>(yr + i) = o;
      }
    } else {
      for (int i = threadIdx.x; i < H; i += blockDim.x)
        yr[i] = f2bf(bf2f(xr[i]) * rstd * bf2f(w[i]));
    }
    __syncthreads();
  }
}

// Residual-add forward (H % 8 == 0 only): the rounded sum is staged in
// dynamic LDS so pass 2 never re-reads global.
__global__ void __launch_bounds__(256) add_rmsnorm_fwd_kernel(
    const short* __restrict__ res, const short* __restrict__ delta,
    const short* __restrict__ w, short* __restrict__ res_out,
    short* __restrict__ y, float* __restrict__ rstd_out, int64_t nrows,
    int H, float eps) {
  __shared__ float scratch[8];
  extern __shared__ short rowbuf[];  // [H] staged res_out (bf16)
  const float invH = 1.0f / (float)H;
  for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const short* rr = res + row * H;
    const short* dr = delta + row * H;
    short* ro = res_out + row * H;
    short* yr = y + row * H;
    float ss = 0.0f;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
      s16x8 rv = *reinterpret_cast<const s16x8*>(rr + i);
      s16x8 dv = *reinterpret_cast<const s16x8*>(dr + i);
      s16x8 sv;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf2f(rv[j]) + bf2f(dv[j]);
        sv[j] = f2bf(f);
        float fq = bf2f(sv[j]);  // accumulate on the ROUNDED value so the
        ss += fq * fq;           // norm matches what res_out stores
      }
      *reinterpret_cast<s16x8*>(ro + i) = sv;
      *reinterpret_cast<s16x8*>(rowbuf + i) = sv;
    }
    ss = block4_sum(ss, scratch);
    const float rstd = rsqrtf(ss * invH + eps);
    if (threadIdx.x == 0 && rstd_out != nullptr) rstd_out[row] = rstd;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
      s16x8 sv = *reinterpret_cast<const s16x8*>(rowbuf + i);
      s16x8 wv = *reinterpret_cast<const s16x8*>(w + i);
      s16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = f2bf(bf2f(sv[j]) * rstd * bf2f(wv[j]));
      *reinterpret_cast<s16x8*>(yr + i) = o;
    }
    __syncthreads();
  }
}

// ---------------- backward: dx + per-block dw partials ----------------
// dw partials accumulate in REGISTERS across this block's rows (each
// thread owns fixed columns) and spill to dw_partial ONCE at the end;
// dy/x rows are staged in dynamic LDS on pass 1 so pass 2 never re-reads
// global. Traffic/row: read dy+x, write dx (the memory-bound floor).
// RES adds the residual gradient dres (streamed in pass 2) to dx; the
// fused op exists for H % 8 == 0 only, so only the plain instantiation
// carries the scalar fallback.
// NCH is the number of 2048-column chunks a thread owns (H <= NCH * 2048):
// pass 2 walks them by a COMPILE-TIME index. With a run-time chunk counter
// the accumulator array is dynamically indexed and the compiler places it
// in private (scratch) memory — a read-modify-write of scratch per element
// that doubled the kernel's traffic.
template <bool RES, int NCH>
__global__ void __launch_bounds__(256) rmsnorm_bwd_kernel(
    const short* __restrict__ dy, const short* __restrict__ dres,
    const short* __restrict__ x, const short* __restrict__ w,
    const float* __restrict__ rstd, short* __restrict__ dx,
    float* __restrict__ dw_partial, int64_t nrows, int H) {
  __shared__ float scratch[8];
  extern __shared__ short rowbuf[];  // [H] dy then [H] x
  short* dy_l = rowbuf;
  short* x_l = rowbuf + H;
  const float invH = 1.0f / (float)H;
  const bool vec = RES || ((H & 7) == 0 && H <= 2048 * 8);
  // per-thread dw accumulators: chunk c covers column i = c*2048 + tid*8
  float dwacc[NCH][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) dwacc[c][j] = 0.0f;

  for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const short* dyr = dy + row * H;
    const short* xr = x + row * H;
    const short* drr = RES ? dres + row * H : nullptr;
    short* dxr = dx + row * H;
    const float rs = rstd[row];
    float dot = 0.0f;
    if (vec) {
      for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        s16x8 dv = *reinterpret_cast<const s16x8*>(dyr + i);
        s16x8 xv = *reinterpret_cast<const s16x8*>(xr + i);
        s16x8 wv = *reinterpret_cast<const s16x8*>(w + i);
        *reinterpret_cast<s16x8*>(dy_l + i) = dv;
        *reinterpret_cast<s16x8*>(x_l + i) = xv;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          dot += bf2f(dv[j]) * bf2f(wv[j]) * bf2f(xv[j]) * rs;
      }
    } else {
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        dy_l[i] = dyr[i];
        x_l[i] = xr[i];
        dot += bf2f(dyr[i]) * bf2f(w[i]) * bf2f(xr[i]) * rs;
      }
    }
    dot = block4_sum(dot, scratch) * invH;
    if (vec) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int i = c * 2048 + threadIdx.x * 8;
        if (i < H) {
          s16x8 dv = *reinterpret_cast<const s16x8*>(dy_l + i);
          s16x8 xv = *reinterpret_cast<const s16x8*>(x_l + i);
          s16x8 wv = *reinterpret_cast<const s16x8*>(w + i);
          s16x8 rv;
          if constexpr (RES)
            rv = *reinterpret_cast<const s16x8*>(drr + i);
          s16x8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float g = bf2f(dv[j]) * bf2f(wv[j]);
            float xhat = bf2f(xv[j]) * rs;
            float d = rs * (g - xhat * dot);
            if constexpr (RES) d += bf2f(rv[j]);
            o[j] = f2bf(d);
            dwacc[c][j] += bf2f(dv[j]) * xhat;
          }
          *reinterpret_cast<s16x8*>(dxr + i) = o;
        }
      }
    } else {
      // scalar fallback: accumulate straight to the partial row (rare)
      float* dwp = dw_partial + (int64_t)blockIdx.x * H;
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        float g = bf2f(dy_l[i]) * bf2f(w[i]);
        float xhat = bf2f(x_l[i]) * rs;
        dxr[i] = f2bf(rs * (g - xhat * dot));
        dwp[i] += bf2f(dy_l[i]) * xhat;
      }
    }
    __syncthreads();
  }
  // spill register accumulators once
  float* dwp = dw_partial + (int64_t)blockIdx.x * H;
  if (vec) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      int i = c * 2048 + threadIdx.x * 8;
      if (i < H) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dwp[i + j] = dwacc[c][j];
      }
    }
  }
}

template <bool RES, int NCH>
static void rmsnorm_bwd_nch(const void* dy, const void* dres, const void* x,
                            const void* w, const void* rstd, void* dx,
                            float* dw_partial, int nblocks, int64_t nrows,
                            int H, hipStream_t s) {
  size_t shmem = 2 * (size_t)H * sizeof(short);
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<RES, NCH>), dim3(nblocks), dim3(256),
                     shmem, s, (const short*)dy, (const short*)dres,
                     (const short*)x, (const short*)w, (const float*)rstd,
                     (short*)dx, dw_partial, nrows, H);
}

template <bool RES>
static void rmsnorm_bwd(const void* dy, const void* dres, const void* x,
                        const void* w, const void* rstd, void* dx,
                        float* dw_partial, void* dw, int nblocks,
                        int64_t nrows, int H, hipStream_t s) {
  // scalar fallback (H not a multiple of 8, or past the 8 register chunks)
  // accumulates into dw_partial directly, so it must start zeroed; the
  // vectorized path overwrites. It keeps no register accumulators, so the
  // one-chunk instantiation serves it.
  const bool scalar = !RES && ((H & 7) || H > 2048 * 8);
  if (scalar)
    (void)hipMemsetAsync(dw_partial, 0, (size_t)nblocks * H * sizeof(float),
                         s);
  const int nch = scalar ? 1 : (H + 2047) / 2048;
#define RMSNORM_BWD_NCH(N)                                                  \
  rmsnorm_bwd_nch<RES, N>(dy, dres, x, w, rstd, dx, dw_partial, nblocks,    \
                          nrows, H, s)
  if (nch <= 1) RMSNORM_BWD_NCH(1);
  else if (nch <= 2) RMSNORM_BWD_NCH(2);
  else if (nch <= 4) RMSNORM_BWD_NCH(4);
  else RMSNORM_BWD_NCH(8);
#undef RMSNORM_BWD_NCH
  colsum_launch(dw_partial, dw, nblocks, H, s);
}

extern "C" {
void rmsnorm_fwd_launch(const void* x, const void* w, void* y, void* rstd,
                        int64_t nrows, int H, float eps, hipStream_t s) {
  hipLaunchKernelGGL(rmsnorm_fwd_kernel, dim3(row_grid(nrows)), dim3(256), 0,
                     s, (const short*)x, (const short*)w, (short*)y,
                     (float*)rstd, nrows, H, eps);
}
void add_rmsnorm_fwd_launch(const void* res, const void* delta, const void* w,
                            void* res_out, void* y, void* rstd, int64_t nrows,
                            int H, float eps, hipStream_t s) {
  size_t shmem = (size_t)H * sizeof(short);
  hipLaunchKernelGGL(add_rmsnorm_fwd_kernel, dim3(row_grid(nrows)), dim3(256),
                     shmem, s, (const short*)res, (const short*)delta,
                     (const short*)w, (short*)res_out, (short*)y, (float*)rstd,
                     nrows, H, eps);
}
void rmsnorm_bwd_launch(const void* dy, const void* x, const void* w,
                        const void* rstd, void* dx, float* dw_partial,
                        void* dw, int nblocks, int64_t nrows, int H,
                        hipStream_t s) {
  rmsnorm_bwd<false>(dy, nullptr, x, w, rstd, dx, dw_partial, dw, nblocks,
                     nrows, H, s);
}
void add_rmsnorm_bwd_launch(const void* dy, const void* dres_out,
                            const void* x, const void* w, const void* rstd,
                            void* dx, float* dw_partial, void* dw,
                            int nblocks, int64_t nrows, int H,
                            hipStream_t s) {
  rmsnorm_bwd<true>(dy, dres_out, x, w, rstd, dx, dw_partial, dw, nblocks,
                    nrows, H, s);
}
}
