// Fused qkv-split + per-head QK RMSNorm + RoPE for gfx950 (Qwen3, OLMo-2,
// Gemma-3 style "QK-norm"): one pass over the packed qkv projection output
// normalises every q and k head row with a learned [D] weight, rotates it
// and writes contiguous q / k / v (forward); one pass re-packs dq/dk/dv into
// dqkv through the inverse rotation and the norm's backward, and leaves the
// weight-gradient partials for colsum.hip (backward).  qkv_rope.hip is the
// same split without the norm and is untouched by this file.
//
// Layouts (as qkv_rope.hip): qkv [B,S,W] bf16, W = (Hq+2*Hkv)*D;
// q [B,S,Hq,D]; k/v [B,S,Hkv,D]; cos/sin f32 [max_pos, D/2]; positions int32
// [S] or null; wq / wk bf16 [D].  D is a template parameter (64, 128: what
// the attention kernels take).
//
// For a q or k head row x (all arithmetic f32, one rounding at the store,
// the convention of norm.hip):
//   r = rsqrt(mean(x^2) + eps), xh = x*r, y = w*xh, out = Rot(y)
//   dy = Rot^T(dout), dx = r*(dy*w - xh*mean(dy*w*xh)), dw += dy*xh
// r and xh are recomputed in the backward from the saved row, which is
// loaded anyway.  v rows (and dv) are copied bit for bit.
//
// Mapping.  A lane owns 8 rotation pairs of one head row: the 16 B at
// column d2 = slot*8 and the 16 B at d2 + D/2, so a row is shared by
// LPR = D/16 adjacent lanes (8 / 4) and a wave pass covers 64/LPR head rows
// (8 / 16) of ONE token.  LPR divides 64: a lane group never straddles a
// wavefront, and the row statistics are a __shfl_xor butterfly over
// log2(LPR) steps: no LDS, no second pass.  A wave walks the tokens
// s = blockIdx.x*4 + wid (+ gridDim.x*4 ...) of batch row blockIdx.y, so
// token, head and column slot come from block, wave and lane: no integer
// divide anywhere (qkv_rope.hip pays three 64-bit ones per 16 elements).
// The token's position and its 16 cos/sin values per lane are loaded once
// per token and serve every head of it.
#include "common.h"
#include "launchers.h"

constexpr int QNR_WAVES = 4;  // 256-thread blocks: tokens per block step

// Each grid is capped at the number of blocks its __launch_bounds__ keeps
// resident on the 256 CUs (forward 4 per CU, backward 3), so every block of
// a capped grid runs from the start and the grid-stride loops share the
// tokens evenly: no second, partly filled round of blocks.
constexpr int QNR_FWD_GRID_CAP = 1024;

// Backward grid cap.  Every block ends with one fold of its 32 per-thread
// dw accumulators (3-4 shuffle steps each, 4 KiB of LDS, one barrier) and
// one [2*D] f32 row for colsum.hip.  With 768 blocks the fold is paid once
// per 32 tokens at the Qwen3-8B layer shape (24576 tokens, 34 KiB of
// traffic each), the partial buffer stays under 1 MiB (0.1 % of the
// kernel's own bytes), and 12 waves per CU with four 16 B loads each keep
// 48 KiB in flight per CU.  Three blocks per CU, not four: with the 32
// accumulators live across the whole kernel a 128-VGPR budget spills
// (48 B of scratch per lane), 168 does not.
constexpr int QNR_BWD_GRID_CAP = 768;

static inline int qnr_grid_x(int64_t B, int S, int cap) {
  int64_t want = ((int64_t)S + QNR_WAVES - 1) / QNR_WAVES;
  int64_t most = cap / (B < 1 ? 1 : B);
  if (most < 1) most = 1;
  if (want > most) want = most;
  return (int)(want < 1 ? 1 : want);
}

__device__ __forceinline__ void load8f(const float* __restrict__ p,
                                       float (&out)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[j] = a[j];
    out[4 + j] = b[j];
  }
}

// sum over the LPR adjacent lanes that share a head row
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

template <int D>
__global__ void __launch_bounds__(256, 4) qkv_norm_rope_fwd_kernel(
    const short* __restrict__ qkv, short* __restrict__ oq,
    short* __restrict__ ok, short* __restrict__ ov,
    const short* __restrict__ wq, const short* __restrict__ wk,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int* __restrict__ positions, int S, int Hq, int Hkv, float eps) {
  constexpr int HALF = D / 2;
  constexpr int LPR = D / 16;
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int d2 = (lane & (LPR - 1)) * 8;
  const int hrow = lane / LPR;
  const int HQK = Hq + Hkv;
  const int HA = HQK + Hkv;
  const int64_t W = (int64_t)HA * D;

  const s16x8 wq0 = *reinterpret_cast<const s16x8*>(wq + d2);
  const s16x8 wq1 = *reinterpret_cast<const s16x8*>(wq + d2 + HALF);
  const s16x8 wk0 = *reinterpret_cast<const s16x8*>(wk + d2);
  const s16x8 wk1 = *reinterpret_cast<const s16x8*>(wk + d2 + HALF);

  for (int s = blockIdx.x * QNR_WAVES + wid; s < S;
       s += gridDim.x * QNR_WAVES) {
    const int64_t tok = (int64_t)blockIdx.y * S + s;
    const int pos = positions ? positions[s] : s;
    float c[8], sv[8];
    load8f(cs + (int64_t)pos * HALF + d2, c);
    load8f(sn + (int64_t)pos * HALF + d2, sv);
    const short* src = qkv + tok * W + d2;
    for (int h0 = 0; h0 < HA; h0 += RPW) {
      const int ha = h0 + hrow;
      const bool live = ha < HA;
      s16x8 v0 = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 v1 = {0, 0, 0, 0, 0, 0, 0, 0};
      if (live) {
        v0 = *reinterpret_cast<const s16x8*>(src + (int64_t)ha * D);
        v1 = *reinterpret_cast<const s16x8*>(src + (int64_t)ha * D + HALF);
      }
      float x0[8], x1[8];
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x0[j] = bf2f(v0[j]);
        x1[j] = bf2f(v1[j]);
        ss += x0[j] * x0[j] + x1[j] * x1[j];
      }
      // every lane of the wave takes part; v rows and idle groups ignore it
      ss = row_sum<LPR>(ss);
      if (!live) continue;
      if (ha < HQK) {  // q or k: norm, weight, rotate
        const bool isq = ha < Hq;
        const float r = rsqrtf(ss * (1.0f / D) + eps);
        const s16x8 w0 = isq ? wq0 : wk0;
        const s16x8 w1 = isq ? wq1 : wk1;
        s16x8 o0, o1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float y0 = bf2f(w0[j]) * (x0[j] * r);
          const float y1 = bf2f(w1[j]) * (x1[j] * r);
          o0[j] = f2bf(y0 * c[j] - y1 * sv[j]);
          o1[j] = f2bf(y0 * sv[j] + y1 * c[j]);
        }
        short* dst = isq ? oq + (tok * Hq + ha) * (int64_t)D
                         : ok + (tok * Hkv + (ha - Hq)) * (int64_t)D;
        *reinterpret_cast<s16x8*>(dst + d2) = o0;
        *reinterpret_cast<s16x8*>(dst + d2 + HALF) = o1;
      } else {  // v: plain copy
        short* dst = ov + (tok * Hkv + (ha - HQK)) * (int64_t)D;
        *reinterpret_cast<s16x8*>(dst + d2) = v0;
        *reinterpret_cast<s16x8*>(dst + d2 + HALF) = v1;
      }
    }
  }
}

template <int D>
__global__ void __launch_bounds__(256, 3) qkv_norm_rope_bwd_kernel(
    const short* __restrict__ dq, const short* __restrict__ dk,
    const short* __restrict__ dv, const short* __restrict__ qkv,
    const short* __restrict__ wq, const short* __restrict__ wk,
    short* __restrict__ dqkv, float* __restrict__ dw_partial,
    const float* __restrict__ cs, const float* __restrict__ sn,
    const int* __restrict__ positions, int S, int Hq, int Hkv, float eps) {
  constexpr int HALF = D / 2;
  constexpr int LPR = D / 16;
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int d2 = (lane & (LPR - 1)) * 8;
  const int hrow = lane / LPR;
  const int HQK = Hq + Hkv;
  const int HA = HQK + Hkv;
  const int64_t W = (int64_t)HA * D;

  // dw accumulators of this lane's 16 columns: one set for q rows, one for
  // k rows, chosen by predication and indexed by unrolled loop variables
  // only (README: a run-time index would move them to scratch)
  float aq0[8], aq1[8], ak0[8], ak1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) aq0[j] = aq1[j] = ak0[j] = ak1[j] = 0.f;

  for (int s = blockIdx.x * QNR_WAVES + wid; s < S;
       s += gridDim.x * QNR_WAVES) {
    const int64_t tok = (int64_t)blockIdx.y * S + s;
    const int pos = positions ? positions[s] : s;
    float c[8], sv[8];
    load8f(cs + (int64_t)pos * HALF + d2, c);
    load8f(sn + (int64_t)pos * HALF + d2, sv);
    for (int h0 = 0; h0 < HA; h0 += RPW) {
      const int ha = h0 + hrow;
      const bool live = ha < HA;
      const bool rot = ha < HQK;  // q or k row (implies live)
      const bool isq = ha < Hq;
      s16x8 g0v = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 g1v = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 v0 = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 v1 = {0, 0, 0, 0, 0, 0, 0, 0};
      if (live) {
        const short* gsrc =
            isq ? dq + (tok * Hq + ha) * (int64_t)D
                : rot ? dk + (tok * Hkv + (ha - Hq)) * (int64_t)D
                      : dv + (tok * Hkv + (ha - HQK)) * (int64_t)D;
        g0v = *reinterpret_cast<const s16x8*>(gsrc + d2);
        g1v = *reinterpret_cast<const s16x8*>(gsrc + d2 + HALF);
      }
      if (rot) {
        const short* xsrc = qkv + tok * W + (int64_t)ha * D + d2;
        v0 = *reinterpret_cast<const s16x8*>(xsrc);
        v1 = *reinterpret_cast<const s16x8*>(xsrc + HALF);
      }
      // The weights are re-read per row (32 B per lane, always an L1 hit)
      // and x, w, dout stay packed between the two loops below (the second
      // repeats the inverse rotation, 4 FMAs a pair): with the 32
      // accumulators live across the whole kernel that keeps the
      // register count down.
      const short* wsrc = (isq ? wq : wk) + d2;
      const s16x8 w0 = *reinterpret_cast<const s16x8*>(wsrc);
      const s16x8 w1 = *reinterpret_cast<const s16x8*>(wsrc + HALF);
      float ss = 0.f, st = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x0 = bf2f(v0[j]);
        const float x1 = bf2f(v1[j]);
        const float g0 = bf2f(g0v[j]);
        const float g1 = bf2f(g1v[j]);
        const float dy0 = g0 * c[j] + g1 * sv[j];
        const float dy1 = -g0 * sv[j] + g1 * c[j];
        ss += x0 * x0 + x1 * x1;
        st += dy0 * bf2f(w0[j]) * x0 + dy1 * bf2f(w1[j]) * x1;
      }
      // two independent butterflies; all lanes take part
      ss = row_sum<LPR>(ss);
      st = row_sum<LPR>(st);
      if (!live) continue;
      short* dst = dqkv + tok * W + (int64_t)ha * D + d2;
      if (rot) {
        const float r = rsqrtf(ss * (1.0f / D) + eps);
        // mean(dy*w*xh) = r * mean(dy*w*x)
        const float mt = r * st * (1.0f / D);
        s16x8 o0, o1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float g0 = bf2f(g0v[j]);
          const float g1 = bf2f(g1v[j]);
          const float dy0 = g0 * c[j] + g1 * sv[j];
          const float dy1 = -g0 * sv[j] + g1 * c[j];
          const float xh0 = bf2f(v0[j]) * r;
          const float xh1 = bf2f(v1[j]) * r;
          o0[j] = f2bf(r * (dy0 * bf2f(w0[j]) - xh0 * mt));
          o1[j] = f2bf(r * (dy1 * bf2f(w1[j]) - xh1 * mt));
          const float t0 = dy0 * xh0;
          const float t1 = dy1 * xh1;
          aq0[j] += isq ? t0 : 0.f;
          aq1[j] += isq ? t1 : 0.f;
          ak0[j] += isq ? 0.f : t0;
          ak1[j] += isq ? 0.f : t1;
        }
        *reinterpret_cast<s16x8*>(dst) = o0;
        *reinterpret_cast<s16x8*>(dst + HALF) = o1;
      } else {  // dv: plain copy
        *reinterpret_cast<s16x8*>(dst) = g0v;
        *reinterpret_cast<s16x8*>(dst + HALF) = g1v;
      }
    }
  }

  // Fold the block's accumulators in a fixed order: a butterfly over the
  // RPW lanes of a wave that own the same columns, then the four waves
  // through LDS.  No atomics: the partial row is bitwise reproducible.
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int off = LPR; off < WAVE; off <<= 1) {
      aq0[j] += __shfl_xor(aq0[j], off, WAVE);
      aq1[j] += __shfl_xor(aq1[j], off, WAVE);
      ak0[j] += __shfl_xor(ak0[j], off, WAVE);
      ak1[j] += __shfl_xor(ak1[j], off, WAVE);
    }
  }
  __shared__ float red[QNR_WAVES][2 * D];
  if (lane < LPR) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[wid][d2 + j] = aq0[j];
      red[wid][HALF + d2 + j] = aq1[j];
      red[wid][D + d2 + j] = ak0[j];
      red[wid][D + HALF + d2 + j] = ak1[j];
    }
  }
  __syncthreads();
  const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int col = threadIdx.x; col < 2 * D; col += blockDim.x)
    dw_partial[blk * (2 * D) + col] =
        (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

extern "C" {
int qkv_norm_rope_bwd_blocks(int64_t B, int S) {
  return (int)(B * qnr_grid_x(B, S, QNR_BWD_GRID_CAP));
}

void qkv_norm_rope_fwd_launch(const void* qkv, const void* wq, const void* wk,
                              void* q, void* k, void* v, const float* cs,
                              const float* sn, const int* positions,
                              int64_t B, int S, int Hq, int Hkv, int D,
                              float eps, hipStream_t stream) {
  if (B < 1 || S < 1) return;
  const dim3 grid(qnr_grid_x(B, S, QNR_FWD_GRID_CAP), (unsigned)B);
  if (D == 128)
    hipLaunchKernelGGL(qkv_norm_rope_fwd_kernel<128>, grid, dim3(256), 0,
                       stream, (const short*)qkv, (short*)q, (short*)k,
                       (short*)v, (const short*)wq, (const short*)wk, cs, sn,
                       positions, S, Hq, Hkv, eps);
  else
    hipLaunchKernelGGL(qkv_norm_rope_fwd_kernel<64>, grid, dim3(256), 0,
                       stream, (const short*)qkv, (short*)q, (short*)k,
                       (short*)v, (const short*)wq, (const short*)wk, cs, sn,
                       positions, S, Hq, Hkv, eps);
}

void qkv_norm_rope_bwd_launch(const void* dq, const void* dk, const void* dv,
                              const void* qkv, const void* wq, const void* wk,
                              void* dqkv, float* dw_partial, void* dw,
                              const float* cs, const float* sn,
                              const int* positions, int64_t B, int S, int Hq,
                              int Hkv, int D, float eps, hipStream_t stream) {
  if (B < 1 || S < 1) return;
  const dim3 grid(qnr_grid_x(B, S, QNR_BWD_GRID_CAP), (unsigned)B);
  if (D == 128)
    hipLaunchKernelGGL(qkv_norm_rope_bwd_kernel<128>, grid, dim3(256), 0,
                       stream, (const short*)dq, (const short*)dk,
                       (const short*)dv, (const short*)qkv, (const short*)wq,
                       (const short*)wk, (short*)dqkv, dw_partial, cs, sn,
                       positions, S, Hq, Hkv, eps);
  else
    hipLaunchKernelGGL(qkv_norm_rope_bwd_kernel<64>, grid, dim3(256), 0,
                       stream, (const short*)dq, (const short*)dk,
                       (const short*)dv, (const short*)qkv, (const short*)wq,
                       (const short*)wk, (short*)dqkv, dw_partial, cs, sn,
                       positions, S, Hq, Hkv, eps);
  colsum_launch(dw_partial, dw, (int)(grid.x * grid.y), 2 * D, stream);
}
}
