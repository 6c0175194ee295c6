// Fused RMSNorm and LayerNorm forward/backward for gfx950; RMSNorm also
// with the residual add folded in.
//
// Replaces the reference's LlamaRMSNorm (transformers; invoked from every
// Llama forward — see SURVEY.md §2b "RMSNorm") and the LayerNorm of HF gpt2
// (the chapter-1 smoke model; SURVEY.md §2b "torch.compile fusions"). One
// workgroup per row, bf16x8 vectorized loads (G13), f32 accumulation,
// wave+block shuffle reductions. Forward saves rstd (and LayerNorm's mu),
// f32 per row, for the backward.
//
// RMSNorm (LN = false):
//   y = x * rsqrt(mean(x^2) + eps) * w
//   dx = rstd * (g - xhat * mean(g * xhat)),  g = dy * w,  xhat = x * rstd
//   dw = sum_rows dy * xhat   (per-block partials, then colsum.hip)
// LayerNorm (LN = true):
//   y  = (x - mu) * rstd * w + b,   rstd = rsqrt(var + eps)
//   dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  xhat = (x - mu) * rstd
//   dw = sum_rows dy * xhat;  db = sum_rows dy
// Where the two differ the arithmetic is written out per norm under
// `if constexpr (LN)`: the expressions associate differently (RMSNorm sums
// d*w*x*rs, LayerNorm g*((x-mu)*rs) on its vector path and g*(x-mu)*rs on
// its scalar path), and merging them would change results in the last bit.
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
// b and mu_out are read / written by the LayerNorm instantiation only.
template <bool LN>
__global__ void __launch_bounds__(256) norm_fwd_kernel(
    const short* __restrict__ x, const short* __restrict__ w,
    const short* __restrict__ b, short* __restrict__ y,
    float* __restrict__ mu_out, float* __restrict__ rstd_out, int64_t nrows,
    int H, float eps) {
  __shared__ float scratch[8];
  __shared__ float mu_sh;
  const float invH = 1.0f / (float)H;
  const bool vec = (H & 7) == 0;
  for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const short* xr = x + row * H;
    short* yr = y + row * H;
    float s = 0.0f, ss = 0.0f;
    if (vec) {
      for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        s16x8 v = *reinterpret_cast<const s16x8*>(xr + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bf2f(v[j]);
          if constexpr (LN) s += f;
          ss += f * f;
        }
      }
    } else {
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        float f = bf2f(xr[i]);
        if constexpr (LN) s += f;
        ss += f * f;
      }
    }
    float mu = 0.0f;
    if constexpr (LN) {
      s = block4_sum(s, scratch);
      if (threadIdx.x == 0) mu_sh = s * invH;
      __syncthreads();
      mu = mu_sh;
    }
    ss = block4_sum(ss, scratch);
    float rstd;
    if constexpr (LN) {
      const float var = ss * invH - mu * mu;
      rstd = rsqrtf(var + eps);
    } else {
      rstd = rsqrtf(ss * invH + eps);
    }
    if (threadIdx.x == 0) {
      if constexpr (LN)
        if (mu_out != nullptr) mu_out[row] = mu;
      if (rstd_out != nullptr) rstd_out[row] = rstd;
    }
    if (vec) {
      for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        s16x8 v = *reinterpret_cast<const s16x8*>(xr + i);
        s16x8 wv = *reinterpret_cast<const s16x8*>(w + i);
        s16x8 bv;
        if constexpr (LN) bv = *reinterpret_cast<const s16x8*>(b + i);
        s16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (LN)
            o[j] = f2bf((bf2f(v[j]) - mu) * rstd * bf2f(wv[j]) + bf2f(bv[j]));
          else
            o[j] = f2bf(bf2f(v[j]) * rstd * bf2f(wv[j]));
        }
        *reinterpret_cast<s16x8*>(yr + i) = o;
      }
    } else {
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        if constexpr (LN)
          yr[i] = f2bf((bf2f(xr[i]) - mu) * rstd * bf2f(w[i]) + bf2f(b[i]));
        else
          yr[i] = f2bf(bf2f(xr[i]) * rstd * bf2f(w[i]));
      }
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

// ---------------- backward: dx + per-block dw (db) partials ----------------
// dw (and LayerNorm's db) partials accumulate in REGISTERS across this
// block's rows (each thread owns fixed columns) and spill to dw_partial /
// db_partial ONCE at the end; dy/x rows are staged in dynamic LDS on pass 1
// so pass 2 never re-reads global. Traffic/row: read dy+x, write dx (the
// memory-bound floor).
// RES adds the residual gradient dres (streamed in pass 2) to dx; the
// fused op exists for RMSNorm at H % 8 == 0 only, so the RES instantiations
// carry no scalar fallback.
// NCH is the number of 2048-column chunks a thread owns (H <= NCH * 2048):
// pass 2 walks them by a COMPILE-TIME index. With a run-time chunk counter
// the accumulator array is dynamically indexed and the compiler places it
// in private (scratch) memory — a read-modify-write of scratch per element
// that doubled the kernel's traffic.

// largest H on the vector path: LayerNorm keeps two accumulator arrays, so
// it stops at four chunks where RMSNorm goes to eight
__host__ __device__ constexpr int norm_bwd_vec_max(bool ln) {
  return 2048 * (ln ? 4 : 8);
}

// mu and db_partial are LayerNorm's and null for RMSNorm.
template <bool LN, bool RES, int NCH>
__global__ void __launch_bounds__(256) norm_bwd_kernel(
    const short* __restrict__ dy, const short* __restrict__ dres,
    const short* __restrict__ x, const short* __restrict__ w,
    const float* __restrict__ rstd, short* __restrict__ dx,
    float* __restrict__ dw_partial, int64_t nrows, int H,
    const float* __restrict__ mu, float* __restrict__ db_partial) {
  static_assert(!(LN && RES), "no fused residual form of LayerNorm");
  __shared__ float scratch[8];
  __shared__ float sh_mg;
  extern __shared__ short rowbuf[];  // [H] dy then [H] x
  short* dy_l = rowbuf;
  short* x_l = rowbuf + H;
  const float invH = 1.0f / (float)H;
  // bound to a constexpr first: called inside the expression below it folds
  // only after inlining, and the loops come out differently (_hip/README.md)
  constexpr int vec_max = norm_bwd_vec_max(LN);
  const bool vec = RES || ((H & 7) == 0 && H <= vec_max);
  // per-thread accumulators: chunk c covers column i = c*2048 + tid*8
  float dwacc[NCH][8], dbacc[LN ? NCH : 1][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dwacc[c][j] = 0.0f;
      if constexpr (LN) dbacc[c][j] = 0.0f;
    }

  for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const short* dyr = dy + row * H;
    const short* xr = x + row * H;
    const short* drr = RES ? dres + row * H : nullptr;
    short* dxr = dx + row * H;
    float m = 0.0f;
    if constexpr (LN) m = mu[row];
    const float rs = rstd[row];
    // pass 1: stage the row, sum g (LayerNorm) and g * xhat over it
    float sg = 0.0f, sgx = 0.0f;
    if (vec) {
      for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        s16x8 dv = *reinterpret_cast<const s16x8*>(dyr + i);
        s16x8 xv = *reinterpret_cast<const s16x8*>(xr + i);
        s16x8 wv = *reinterpret_cast<const s16x8*>(w + i);
        *reinterpret_cast<s16x8*>(dy_l + i) = dv;
        *reinterpret_cast<s16x8*>(x_l + i) = xv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (LN) {
            float g = bf2f(dv[j]) * bf2f(wv[j]);
            float xhat = (bf2f(xv[j]) - m) * rs;
            sg += g;
            sgx += g * xhat;
          } else {
            sgx += bf2f(dv[j]) * bf2f(wv[j]) * bf2f(xv[j]) * rs;
          }
        }
      }
    } else {
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        dy_l[i] = dyr[i];
        x_l[i] = xr[i];
        if constexpr (LN) {
          float g = bf2f(dyr[i]) * bf2f(w[i]);
          sg += g * 1.0f;
          sgx += g * (bf2f(xr[i]) - m) * rs;
        } else {
          sgx += bf2f(dyr[i]) * bf2f(w[i]) * bf2f(xr[i]) * rs;
        }
      }
    }
    float mg = 0.0f;
    if constexpr (LN) {
      sg = block4_sum(sg, scratch);
      if (threadIdx.x == 0) sh_mg = sg * invH;
      __syncthreads();
      mg = sh_mg;
    }
    const float mgx = block4_sum(sgx, scratch) * invH;
    // pass 2: dx from the staged row, accumulate this row's dw (db) terms
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
            if constexpr (LN) {
              float d = bf2f(dv[j]);
              float g = d * bf2f(wv[j]);
              float xhat = (bf2f(xv[j]) - m) * rs;
              o[j] = f2bf(rs * (g - mg - xhat * mgx));
              dwacc[c][j] += d * xhat;
              dbacc[c][j] += d;
            } else {
              float g = bf2f(dv[j]) * bf2f(wv[j]);
              float xhat = bf2f(xv[j]) * rs;
              float d = rs * (g - xhat * mgx);
              if constexpr (RES) d += bf2f(rv[j]);
              o[j] = f2bf(d);
              dwacc[c][j] += bf2f(dv[j]) * xhat;
            }
          }
          *reinterpret_cast<s16x8*>(dxr + i) = o;
        }
      }
    } else {
      // scalar fallback: accumulate straight to the partial rows (rare)
      float* dwp = dw_partial + (int64_t)blockIdx.x * H;
      float* dbp = LN ? db_partial + (int64_t)blockIdx.x * H : nullptr;
      for (int i = threadIdx.x; i < H; i += blockDim.x) {
        if constexpr (LN) {
          float d = bf2f(dy_l[i]);
          float g = d * bf2f(w[i]);
          float xhat = (bf2f(x_l[i]) - m) * rs;
          dxr[i] = f2bf(rs * (g - mg - xhat * mgx));
          dwp[i] += d * xhat;
          dbp[i] += d;
        } else {
          float g = bf2f(dy_l[i]) * bf2f(w[i]);
          float xhat = bf2f(x_l[i]) * rs;
          dxr[i] = f2bf(rs * (g - xhat * mgx));
          dwp[i] += bf2f(dy_l[i]) * xhat;
        }
      }
    }
    __syncthreads();
  }
  // spill register accumulators once
  float* dwp = dw_partial + (int64_t)blockIdx.x * H;
  float* dbp = LN ? db_partial + (int64_t)blockIdx.x * H : nullptr;
  if (vec) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      int i = c * 2048 + threadIdx.x * 8;
      if (i < H) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          dwp[i + j] = dwacc[c][j];
          if constexpr (LN) dbp[i + j] = dbacc[c][j];
        }
      }
    }
  }
}

// picks the instantiation for nch chunks; LayerNorm's vector path ends at 4
template <bool LN, bool RES>
static void norm_bwd_nch(const short* dy, const short* dres, const short* x,
                         const short* w, const float* mu, const float* rstd,
                         short* dx, float* dw_partial, float* db_partial,
                         int nch, int nblocks, int64_t nrows, int H,
                         hipStream_t s) {
  const size_t shmem = 2 * (size_t)H * sizeof(short);
#define NORM_BWD_NCH(N)                                                     \
  hipLaunchKernelGGL((norm_bwd_kernel<LN, RES, N>), dim3(nblocks),          \
                     dim3(256), shmem, s, dy, dres, x, w, rstd, dx,         \
                     dw_partial, nrows, H, mu, db_partial)
  if (nch <= 1) NORM_BWD_NCH(1);
  else if (nch <= 2) NORM_BWD_NCH(2);
  else if (LN || nch <= 4) NORM_BWD_NCH(4);
  else if constexpr (!LN) NORM_BWD_NCH(8);
#undef NORM_BWD_NCH
}

extern "C" {
void norm_fwd_launch(const void* x, const void* w, const void* b, void* y,
                     float* mu, float* rstd, int64_t nrows, int H, float eps,
                     hipStream_t s) {
#define NORM_FWD(LN)                                                        \
  hipLaunchKernelGGL(norm_fwd_kernel<LN>, dim3(row_grid(nrows)), dim3(256), \
                     0, s, (const short*)x, (const short*)w,                \
                     (const short*)b, (short*)y, mu, rstd, nrows, H, eps)
  if (mu != nullptr) NORM_FWD(true);
  else NORM_FWD(false);
#undef NORM_FWD
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

void norm_bwd_launch(const void* dy, const void* dres, const void* x,
                     const void* w, const float* mu, const float* rstd,
                     void* dx, float* dw_partial, float* db_partial, void* dw,
                     void* db, int nblocks, int64_t nrows, int H,
                     hipStream_t s) {
  const bool ln = mu != nullptr, res = dres != nullptr;
  // scalar fallback (H not a multiple of 8, or past the register chunks)
  // accumulates into the partials directly, so they must start zeroed; the
  // vectorized path overwrites. It keeps no register accumulators, so the
  // one-chunk instantiation serves it.
  const bool scalar = !res && ((H & 7) || H > norm_bwd_vec_max(ln));
  if (nblocks > 0) {  // zero rows: no grid to launch, colsum writes zeros
    const size_t pbytes = (size_t)nblocks * H * sizeof(float);
    if (scalar) {
      (void)hipMemsetAsync(dw_partial, 0, pbytes, s);
      if (ln) (void)hipMemsetAsync(db_partial, 0, pbytes, s);
    }
    const int nch = scalar ? 1 : (H + 2047) / 2048;
#define NORM_BWD(LN, RES)                                                   \
  norm_bwd_nch<LN, RES>((const short*)dy, (const short*)dres,               \
                        (const short*)x, (const short*)w, mu, rstd,         \
                        (short*)dx, dw_partial, db_partial, nch, nblocks,   \
                        nrows, H, s)
    if (ln) NORM_BWD(true, false);
    else if (res) NORM_BWD(false, true);
    else NORM_BWD(false, false);
#undef NORM_BWD
  }
  colsum_launch(dw_partial, dw, nblocks, H, s);
  // keyed on db, not on ln: with zero rows LayerNorm's empty `mu` is a null
  // pointer too, and db must still come out as zeros
  if (db) colsum_launch(db_partial, db, nblocks, H, s);
}
}
