// Mixture-of-experts token dispatch for gfx950: the expert-sorted row layout
// that a grouped GEMM takes, built on the device, and the two row movers
// around the expert GEMMs (ops/moe.py).
//
// Slot s = t*k + j is token t's j-th selected expert, e = topk_idx[s].  The
// layout is the stable sort of the slots by expert: dest[s] is the slot's
// row, rows of one expert are contiguous and ordered by s, and offs[e] is
// the inclusive cumulative row count per expert.
//
// Index build: three launches, no atomics, no pre-zeroed buffer, no host
// sync, bitwise reproducible (the shape of grad_norm.hip).
//   1. hist    every wave owns one contiguous span of slots and counts its
//              experts into hist[e][wave], written by ordinary stores.
//   2. scan    one 1024-thread block turns hist, read expert-major, into its
//              exclusive prefix in place: entry (e, wave) becomes the first
//              row of that wave's slots of expert e.  It also writes offs.
//   3. rank    every wave walks its span again, 64 slots a step, and hands
//              out rows in slot order.
// Steps 1 and 3 share one idiom.  The lanes of a step that hold the same
// expert find each other with log2(E) ballots (the AND over the expert's
// bits of "ballot or its complement"); a slot's rank among them is the
// popcount of that mask below its lane, and the group's lowest lane alone
// moves the wave's private LDS counter.  One writer per counter per step:
// nothing to make atomic.
//
// Row movers: one wave per token, a lane owns 16 B (8 bf16) of the row per
// 1 KiB column step; every lane loads the token's k destination rows (and
// weights) itself, from k wave-uniform addresses, before it enters the
// column loop, so no lane depends on another being active.  Token, slot
// and column come from block, wave and lane: no integer divide.  The loops
// over j are unrolled to MOE_MAX_K under a j < k predicate, so the per-slot
// accumulators are registers, never indexed at run time.
//   scatter   xp[dest[s], :] = x[t, :], a bit-exact copy; dest is a
//             permutation, so every row of xp is written exactly once and
//             nothing is cleared first.  Given a weight table it is the
//             combine's backward: dyp[dest[s], :] = w[s] * dy[t, :], and in
//             the same pass dw[s] = <dy[t, :], yp[dest[s], :]> by an f32
//             wave reduction, dy[t] being read once for its k slots.
//   combine   y[t, :] = sum_j w[t, j] * yp[dest[t*k + j], :], f32 in fixed
//             j order, rounded once.  A null weight table means weights of
//             one: the scatter's backward, dx[t] = sum_j dxp[dest[t*k + j]].
#include "common.h"
#include "launchers.h"

constexpr int MD_WAVES = 4;        // waves per block of the hist / rank passes
constexpr int MD_MAX_BLOCKS = 64;  // so at most 256 waves, 32768 scan entries
constexpr int MD_MIN_SPAN = 256;   // slots a wave takes at least
constexpr int MD_SCAN_THREADS = 1024;
constexpr int MD_MAX_E = 128;
constexpr int MD_ROW_GRID_CAP = 4096;

struct MdPlan {
  int blocks;  // grid of hist / rank; blocks * MD_WAVES spans
  int span;    // slots per wave, a multiple of 64
};

static inline MdPlan md_plan(int64_t N) {
  int64_t blocks = (N + MD_WAVES * MD_MIN_SPAN - 1) / (MD_WAVES * MD_MIN_SPAN);
  blocks = blocks < 1 ? 1 : blocks > MD_MAX_BLOCKS ? MD_MAX_BLOCKS : blocks;
  const int64_t waves = blocks * MD_WAVES;
  int64_t span = (N + waves - 1) / waves;
  span = (span + WAVE - 1) / WAVE * WAVE;
  return {(int)blocks, (int)(span < WAVE ? WAVE : span)};
}

// Mask of the wave's lanes that hold the same expert as this one; lanes with
// live == false match nobody and get 0.
template <int EBITS>
__device__ __forceinline__ uint64_t same_expert_mask(int e, bool live) {
  uint64_t mask = __ballot(live);
#pragma unroll
  for (int b = 0; b < EBITS; ++b) {
    const bool bit = (e >> b) & 1;
    const uint64_t has = __ballot(bit);
    mask &= bit ? has : ~has;
  }
  return live ? mask : 0ull;
}

// One 64-slot step of a wave over its private LDS counters `cnt`: returns
// the lane's row (counter before the step plus its rank in the step) and
// advances the counters.  The counters belong to this wave alone, and a
// wave's LDS instructions execute in program order, so the step's loads, its
// one store per expert and the next step's loads need no block barrier: the
// wavefront-scope fences only keep the compiler from moving or merging the
// accesses across them.  The four waves of a block never wait for each other.
__device__ __forceinline__ void md_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int EBITS>
__device__ __forceinline__ int md_step(int* cnt, int e, bool live, int lane) {
  const uint64_t mask = same_expert_mask<EBITS>(e, live);
  const uint64_t below = mask & ((1ull << lane) - 1ull);
  int first = 0;
  if (live) first = cnt[e];
  md_wave_fence();
  if (live && below == 0ull) cnt[e] = first + __popcll(mask);
  md_wave_fence();
  return first + __popcll(below);
}

template <int EBITS>
__global__ void __launch_bounds__(256) moe_hist_kernel(
    const int* __restrict__ topk_idx, int* __restrict__ hist, int64_t N,
    int span) {
  constexpr int E = 1 << EBITS;
  __shared__ int cnt_all[MD_WAVES][E];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int gw = blockIdx.x * MD_WAVES + wid;
  const int nw = gridDim.x * MD_WAVES;
  int* cnt = cnt_all[wid];
  for (int e = lane; e < E; e += WAVE) cnt[e] = 0;
  __syncthreads();
  const int64_t base = (int64_t)gw * span;
  for (int i = 0; i < span; i += WAVE) {
    const int64_t s = base + i + lane;
    const bool live = s < N;
    int e = live ? topk_idx[s] : 0;
    DTGA_KERNEL_ASSERT(e >= 0 && e < E);
    e &= E - 1;  // a corrupt index must not leave the counters
    md_step<EBITS>(cnt, e, live, lane);
  }
  for (int e = lane; e < E; e += WAVE) hist[(int64_t)e * nw + gw] = cnt[e];
}

// <<<1, 1024>>>: exclusive prefix of hist[0 .. n) in place (n = E * nw,
// expert-major), and offs[e] = rows of experts 0..e.  A thread owns `per`
// adjacent entries; the thread totals are scanned by wave shuffles and one
// pass over the 16 wave totals.
__global__ void __launch_bounds__(MD_SCAN_THREADS) moe_scan_kernel(
    int* __restrict__ hist, int* __restrict__ offs, int n, int nw, int E,
    int total) {
  __shared__ int wave_tot[MD_SCAN_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int per = (n + MD_SCAN_THREADS - 1) / MD_SCAN_THREADS;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < n ? lo + per : n;
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += hist[i];
  // inclusive scan of the thread totals inside the wave
  int incl = sum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int up = __shfl_up(incl, off, WAVE);
    if (lane >= off) incl += up;
  }
  if (lane == WAVE - 1) wave_tot[wid] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wid; ++w) before += wave_tot[w];
  int run = before + incl - sum;
  for (int i = lo; i < hi; ++i) {
    const int c = hist[i];
    hist[i] = run;
    run += c;
  }
  __threadfence_block();
  __syncthreads();
  // expert e ends where expert e+1 begins
  if ((int)threadIdx.x < E)
    offs[threadIdx.x] =
        (int)threadIdx.x + 1 < E ? hist[((int)threadIdx.x + 1) * nw] : total;
}

template <int EBITS>
__global__ void __launch_bounds__(256) moe_rank_kernel(
    const int* __restrict__ topk_idx, const int* __restrict__ hist,
    int* __restrict__ dest, int64_t N, int span) {
  constexpr int E = 1 << EBITS;
  __shared__ int cnt_all[MD_WAVES][E];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int gw = blockIdx.x * MD_WAVES + wid;
  const int nw = gridDim.x * MD_WAVES;
  int* cnt = cnt_all[wid];
  for (int e = lane; e < E; e += WAVE) cnt[e] = hist[(int64_t)e * nw + gw];
  __syncthreads();
  const int64_t base = (int64_t)gw * span;
  for (int i = 0; i < span; i += WAVE) {
    const int64_t s = base + i + lane;
    const bool live = s < N;
    int e = live ? topk_idx[s] : 0;
    e &= E - 1;
    const int row = md_step<EBITS>(cnt, e, live, lane);
    if (live) dest[s] = row;
  }
}

// ---- row movers ----
constexpr int MOE_MAX_K = 8;

// Token t's k destination rows and router weights, loaded by every lane from
// the same k addresses before the column loop, where all 64 lanes are
// active.  Nothing is passed between lanes, so a lane that owns no column of
// a narrow row (H < 512) cannot leave another lane without its row.  The
// indices are compile-time after unrolling: registers, no scratch.
struct MdSlots {
  int row[MOE_MAX_K];
  float w[MOE_MAX_K];
};

template <bool WEIGHTED>
__device__ __forceinline__ MdSlots md_load_slots(const int* __restrict__ dest,
                                                 const float* __restrict__ w,
                                                 int64_t t, int k) {
  MdSlots sl;
#pragma unroll
  for (int j = 0; j < MOE_MAX_K; ++j) {
    // all lanes hold the same value; readfirstlane tells the compiler so
    // and the 16 values live in scalar registers
    sl.row[j] = __builtin_amdgcn_readfirstlane(j < k ? dest[t * k + j] : 0);
    sl.w[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(
        (WEIGHTED && j < k) ? w[t * k + j] : 1.f)));
  }
  return sl;
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(256) moe_scatter_kernel(
    const short* __restrict__ x, const int* __restrict__ dest,
    const float* __restrict__ w, const short* __restrict__ yp,
    short* __restrict__ xp, float* __restrict__ dw, int64_t T, int H, int k) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  for (int64_t t = (int64_t)blockIdx.x * MD_WAVES + wid; t < T;
       t += (int64_t)gridDim.x * MD_WAVES) {
    const MdSlots sl = md_load_slots<WEIGHTED>(dest, w, t, k);
    float acc[MOE_MAX_K];
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; ++j) acc[j] = 0.f;
    const short* src = x + t * H;
    for (int c = lane * 8; c < H; c += WAVE * 8) {
      const s16x8 v = *reinterpret_cast<const s16x8*>(src + c);
#pragma unroll
      for (int j = 0; j < MOE_MAX_K; ++j) {
        if (j < k) {
          const int64_t row = (int64_t)sl.row[j] * H + c;
          if (WEIGHTED) {
            const float wj = sl.w[j];
            const s16x8 u = *reinterpret_cast<const s16x8*>(yp + row);
            s16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float f = bf2f(v[i]);
              acc[j] += f * bf2f(u[i]);
              o[i] = f2bf(wj * f);
            }
            *reinterpret_cast<s16x8*>(xp + row) = o;
          } else {
            *reinterpret_cast<s16x8*>(xp + row) = v;
          }
        }
      }
    }
    if (WEIGHTED) {
#pragma unroll
      for (int j = 0; j < MOE_MAX_K; ++j) {
        if (j < k) {
          const float r = wave_reduce_sum(acc[j]);
          if (lane == 0) dw[t * k + j] = r;
        }
      }
    }
  }
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(256) moe_combine_kernel(
    const short* __restrict__ yp, const int* __restrict__ dest,
    const float* __restrict__ w, short* __restrict__ y, int64_t T, int H,
    int k) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  for (int64_t t = (int64_t)blockIdx.x * MD_WAVES + wid; t < T;
       t += (int64_t)gridDim.x * MD_WAVES) {
    const MdSlots sl = md_load_slots<WEIGHTED>(dest, w, t, k);
    for (int c = lane * 8; c < H; c += WAVE * 8) {
      float a[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) a[i] = 0.f;
#pragma unroll
      for (int j = 0; j < MOE_MAX_K; ++j) {
        if (j < k) {
          const int64_t row = (int64_t)sl.row[j] * H + c;
          const s16x8 u = *reinterpret_cast<const s16x8*>(yp + row);
          if (WEIGHTED) {
            const float wj = sl.w[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] += wj * bf2f(u[i]);
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] += bf2f(u[i]);
          }
        }
      }
      s16x8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = f2bf(a[i]);
      *reinterpret_cast<s16x8*>(y + t * H + c) = o;
    }
  }
}

static inline int md_row_grid(int64_t T) {
  const int64_t want = (T + MD_WAVES - 1) / MD_WAVES;
  return (int)(want < 1 ? 1 : want < MD_ROW_GRID_CAP ? want : MD_ROW_GRID_CAP);
}

#define MD_BY_EBITS(KERNEL, ...)                                             \
  switch (E) {                                                               \
    case 8: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, s, __VA_ARGS__); break;   \
    case 16: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, s, __VA_ARGS__); break;  \
    case 32: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(256), 0, s, __VA_ARGS__); break;  \
    case 64: hipLaunchKernelGGL(KERNEL<6>, grid, dim3(256), 0, s, __VA_ARGS__); break;  \
    case 128: hipLaunchKernelGGL(KERNEL<7>, grid, dim3(256), 0, s, __VA_ARGS__); break; \
    default: break; /* the binding rejects every other E */                  \
  }

extern "C" {
int64_t moe_index_scratch(int64_t N, int E) {
  return (int64_t)E * md_plan(N).blocks * MD_WAVES;
}

void moe_index_launch(const int* topk_idx, int* dest, int* offs, int* hist,
                      int64_t N, int E, hipStream_t s) {
  static_assert(MD_MAX_E * MD_MAX_BLOCKS * MD_WAVES <=
                    MD_SCAN_THREADS * 32, "scan entries per thread");
  const MdPlan p = md_plan(N);
  const dim3 grid(p.blocks);
  const int nw = p.blocks * MD_WAVES;
  MD_BY_EBITS(moe_hist_kernel, topk_idx, hist, N, p.span);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(MD_SCAN_THREADS), 0, s,
                     hist, offs, E * nw, nw, E, (int)N);
  MD_BY_EBITS(moe_rank_kernel, topk_idx, (const int*)hist, dest, N, p.span);
}

void moe_scatter_launch(const void* x, const int* dest, const float* w,
                        const void* yp, void* xp, float* dw, int64_t T, int H,
                        int k, hipStream_t s) {
  if (T < 1) return;
  const dim3 grid(md_row_grid(T));
  if (w)
    hipLaunchKernelGGL(moe_scatter_kernel<true>, grid, dim3(256), 0, s,
                       (const short*)x, dest, w, (const short*)yp, (short*)xp,
                       dw, T, H, k);
  else
    hipLaunchKernelGGL(moe_scatter_kernel<false>, grid, dim3(256), 0, s,
                       (const short*)x, dest, w, (const short*)yp, (short*)xp,
                       dw, T, H, k);
}

void moe_combine_launch(const void* yp, const int* dest, const float* w,
                        void* y, int64_t T, int H, int k, hipStream_t s) {
  if (T < 1) return;
  const dim3 grid(md_row_grid(T));
  if (w)
    hipLaunchKernelGGL(moe_combine_kernel<true>, grid, dim3(256), 0, s,
                       (const short*)yp, dest, w, (short*)y, T, H, k);
  else
    hipLaunchKernelGGL(moe_combine_kernel<false>, grid, dim3(256), 0, s,
                       (const short*)yp, dest, w, (short*)y, T, H, k);
}
}
