// Sorted embedding backward for gfx950: dtable[v] = sum of dy[r] over the
// flat positions r with ids[r] == v, accumulated in f32 in an order that is
// a function of ids and the shapes alone, rounded to bf16 once.  No atomics,
// no cleared buffer, no f32 [V, H] workspace, no host sync; every row of
// dtable is written exactly once, rows that no token hits as zeros by the
// kernel that writes the sums (embedding.hip's scatter is the atomic form).
//
//   1. sort   stable LSD radix sort of the positions by id, ceil(log2 V) bits
//             in passes of at most 9 (two passes up to V = 2^18).  A pass is
//             the index build of moe_dispatch.hip: every wave owns one
//             contiguous span of keys and counts its digits into
//             hist[digit][wave] by ordinary stores; one 1024-thread block
//             turns hist, read digit-major, into its exclusive prefix; every
//             wave walks its span again and hands out destinations in span
//             order.  Lanes of a step with the same digit find each other
//             with ballots, and the group's lowest lane alone moves the
//             wave's private LDS counter, between wavefront-scope fences.
//             The first pass narrows the int64 ids to int32 keys; the
//             position travels as the payload.
//   2. seg    seg[v], v = 0..V: first sorted index whose key is >= v, one
//             thread per v by binary search over the sorted keys.
//   3. chunk  the sorted index space is cut into slots of ES_CHUNK.  A row
//             whose occurrences [seg[v], seg[v+1]) run past the end of the
//             slot they start in is cut there and at every later slot
//             boundary.  Slot k >= 1 therefore holds at most one piece that
//             begins at k * ES_CHUNK in the middle of a row, and that piece
//             is summed here into partial row k - 1 (f32), by one wave per
//             (slot, 1 KiB column step): a row of any length is summed by as
//             many waves as it has pieces and column steps.
//   4. fold   the cut rows, again one wave per (slot boundary, column step):
//             the wave at the first boundary a row crosses sums the row's
//             head (its occurrences before that boundary, at most ES_CHUNK)
//             in sorted order, adds the row's partials in slot order, 8 in
//             flight, rounds and stores its 1 KiB of the row.  Launches 3
//             and 4 are a work list of pieces that needs no building: its
//             entries are the slot boundaries, and a boundary that cuts no
//             row costs four loads.
//   5. row    a wave owns a vocabulary row per step and skips the cut ones:
//             it sums the row's occurrences (at most ES_CHUNK) in sorted
//             order, rounds and stores 16 B per lane per column step.  An
//             empty row has nothing to sum and stores zeros.
// Which slot boundaries cut a row follows from ids alone, so the order of
// summation does too.  Scratch: 4N + 512 * waves + V + 1 ints and
// ceil(N / ES_CHUNK) - 1 f32 rows.
//
// A lane keeps 8 f32 accumulators, its 8 columns of a 512-column step,
// indexed at compile time only.  With H % 8 == 0 and 16 B aligned rows those
// are 8 adjacent columns (one 16 B load per hit, 8 hits in flight);
// otherwise columns c0 + j * 64 + lane, loaded one bf16 at a time.
#include "common.h"
#include "launchers.h"

constexpr int ES_WAVES = 4;        // waves per block, every kernel but the scan
constexpr int ES_MAX_BLOCKS = 64;  // so at most 256 sorting waves
constexpr int ES_MIN_SPAN = 256;   // keys a sorting wave takes at least
constexpr int ES_SCAN_THREADS = 1024;
constexpr int ES_MAX_DBITS = 9;    // digit width: 512 counters per wave
constexpr int ES_LOG2_CHUNK = 7;
constexpr int ES_CHUNK = 1 << ES_LOG2_CHUNK;
constexpr int ES_COLS = WAVE * 8;  // columns of a wave's column step
constexpr int ES_INFLIGHT = 8;     // hits loaded before the first is added
constexpr int ES_ROW_GRID_CAP = 65536;

struct EsPlan {
  int blocks;  // grid of hist / rank; blocks * ES_WAVES spans
  int span;    // keys per wave, a multiple of 64
  int bits;    // key bits, at least 1
  int npass;
};

static inline EsPlan es_plan(int64_t N, int64_t V) {
  int64_t blocks = (N + ES_WAVES * ES_MIN_SPAN - 1) / (ES_WAVES * ES_MIN_SPAN);
  blocks = blocks < 1 ? 1 : blocks > ES_MAX_BLOCKS ? ES_MAX_BLOCKS : blocks;
  const int64_t waves = blocks * ES_WAVES;
  int64_t span = (N + waves - 1) / waves;
  span = (span + WAVE - 1) / WAVE * WAVE;
  int bits = 1;
  while (((int64_t)1 << bits) < V) ++bits;
  return {(int)blocks, (int)(span < WAVE ? WAVE : span), bits,
          (bits + ES_MAX_DBITS - 1) / ES_MAX_DBITS};
}

__device__ __forceinline__ void es_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One 64-key step of a wave over its private LDS counters: returns the
// lane's destination (counter before the step plus its rank among the
// step's lanes with the same digit) and advances the counters.  One writer
// per counter per step, so nothing is atomic; the counters belong to this
// wave alone and a wave's LDS instructions execute in order, so the fences
// only keep the compiler from moving the accesses across them.
__device__ __forceinline__ int es_step(int* cnt, int d, int dbits, bool live,
                                       int lane) {
  uint64_t mask = __ballot(live);
  for (int b = 0; b < dbits; ++b) {
    const bool bit = (d >> b) & 1;
    const uint64_t has = __ballot(bit);
    mask &= bit ? has : ~has;
  }
  if (!live) mask = 0ull;
  const uint64_t below = mask & ((1ull << lane) - 1ull);
  int first = 0;
  if (live) first = cnt[d];
  es_wave_fence();
  if (live && below == 0ull) cnt[d] = first + __popcll(mask);
  es_wave_fence();
  return first + __popcll(below);
}

// The key at sorted-so-far index s: the id itself in the first pass, masked
// to the key bits so that an id outside the contract can reach neither
// another counter nor, later, another row's memory.
template <bool FIRST>
__device__ __forceinline__ int es_key(const int64_t* __restrict__ ids,
                                      const int* __restrict__ keys, int64_t s,
                                      int keymask, int64_t V) {
  if (FIRST) {
    const int64_t id = ids[s];
    DTGA_KERNEL_ASSERT(id >= 0 && id < V);
    return (int)id & keymask;
  }
  return keys[s];
}

template <bool FIRST>
__global__ void __launch_bounds__(256) embed_sort_hist_kernel(
    const int64_t* __restrict__ ids, const int* __restrict__ keys,
    int* __restrict__ hist, int64_t N, int span, int shift, int dbits,
    int keymask, int64_t V) {
  __shared__ int cnt_all[ES_WAVES][1 << ES_MAX_DBITS];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int gw = blockIdx.x * ES_WAVES + wid;
  const int nw = gridDim.x * ES_WAVES;
  const int D = 1 << dbits;
  int* cnt = cnt_all[wid];
  for (int d = lane; d < D; d += WAVE) cnt[d] = 0;
  __syncthreads();
  const int64_t base = (int64_t)gw * span;
  for (int i = 0; i < span; i += WAVE) {
    const int64_t s = base + i + lane;
    const bool live = s < N;
    const int key = live ? es_key<FIRST>(ids, keys, s, keymask, V) : 0;
    es_step(cnt, (key >> shift) & (D - 1), dbits, live, lane);
  }
  for (int d = lane; d < D; d += WAVE) hist[(int64_t)d * nw + gw] = cnt[d];
}

// <<<1, 1024>>>: exclusive prefix of hist[0 .. n) in place (n = digits *
// waves, digit-major).  A thread owns `per` adjacent entries; the thread
// totals are scanned by wave shuffles and one pass over the 16 wave totals.
__global__ void __launch_bounds__(ES_SCAN_THREADS) embed_sort_scan_kernel(
    int* __restrict__ hist, int n) {
  __shared__ int wave_tot[ES_SCAN_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int per = (n + ES_SCAN_THREADS - 1) / ES_SCAN_THREADS;
  const int lo = threadIdx.x * per < n ? threadIdx.x * per : n;
  const int hi = lo + per < n ? lo + per : n;
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += hist[i];
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
}

template <bool FIRST>
__global__ void __launch_bounds__(256) embed_sort_rank_kernel(
    const int64_t* __restrict__ ids, const int* __restrict__ keys,
    const int* __restrict__ pos, const int* __restrict__ hist,
    int* __restrict__ keys_out, int* __restrict__ pos_out, int64_t N, int span,
    int shift, int dbits, int keymask, int64_t V) {
  __shared__ int cnt_all[ES_WAVES][1 << ES_MAX_DBITS];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int gw = blockIdx.x * ES_WAVES + wid;
  const int nw = gridDim.x * ES_WAVES;
  const int D = 1 << dbits;
  int* cnt = cnt_all[wid];
  for (int d = lane; d < D; d += WAVE) cnt[d] = hist[(int64_t)d * nw + gw];
  __syncthreads();
  const int64_t base = (int64_t)gw * span;
  for (int i = 0; i < span; i += WAVE) {
    const int64_t s = base + i + lane;
    const bool live = s < N;
    const int key = live ? es_key<FIRST>(ids, keys, s, keymask, V) : 0;
    const int to = es_step(cnt, (key >> shift) & (D - 1), dbits, live, lane);
    if (live) {
      keys_out[to] = key;
      pos_out[to] = FIRST ? (int)s : pos[s];
    }
  }
}

__global__ void __launch_bounds__(256) embed_seg_kernel(
    const int* __restrict__ keys, int* __restrict__ seg, int N, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > V) return;
  int lo = 0, hi = N;  // first index in [0, N] whose key is >= v
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  seg[v] = lo;
}

// a += dy[order[i], the lane's columns of step c0] for i = lo .. hi - 1, in
// that order.  lo, hi and every order[i] are the same in all lanes.
template <bool VEC>
__device__ __forceinline__ void es_sum_hits(const short* __restrict__ dy,
                                            const int* __restrict__ order,
                                            int lo, int hi, int H, int c0,
                                            int lane, float (&a)[8]) {
  int i = lo;
  if (VEC) {
    const int c = c0 + lane * 8;
    const bool on = c < H;
    const s16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (; i + ES_INFLIGHT <= hi; i += ES_INFLIGHT) {
      s16x8 v[ES_INFLIGHT];
#pragma unroll
      for (int u = 0; u < ES_INFLIGHT; ++u) {
        const int p = __builtin_amdgcn_readfirstlane(order[i + u]);
        v[u] = on ? *reinterpret_cast<const s16x8*>(dy + (int64_t)p * H + c)
                  : zero;
      }
#pragma unroll
      for (int u = 0; u < ES_INFLIGHT; ++u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += bf2f(v[u][j]);
      }
    }
    for (; i < hi; ++i) {
      const int p = __builtin_amdgcn_readfirstlane(order[i]);
      const s16x8 v =
          on ? *reinterpret_cast<const s16x8*>(dy + (int64_t)p * H + c) : zero;
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += bf2f(v[j]);
    }
  } else {
    for (; i < hi; ++i) {
      const int p = __builtin_amdgcn_readfirstlane(order[i]);
      const short* src = dy + (int64_t)p * H;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j * WAVE + lane;
        if (c < H) a[j] += bf2f(src[c]);
      }
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) embed_chunk_kernel(
    const short* __restrict__ dy, const int* __restrict__ order,
    const int* __restrict__ keys, const int* __restrict__ seg,
    float* __restrict__ part, int H, int64_t V) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int c0 = ((int)blockIdx.y * ES_WAVES + wid) * ES_COLS;
  if (c0 >= H) return;
  const int k = (int)blockIdx.x + 1;
  const int lo = k << ES_LOG2_CHUNK;
  const int v = __builtin_amdgcn_readfirstlane(keys[lo]);
  if (v >= V) return;  // an id outside the contract owns no row
  // a row that starts at or after lo has its head here: the row kernel's
  if (__builtin_amdgcn_readfirstlane(seg[v]) >= lo) return;
  const int e = __builtin_amdgcn_readfirstlane(seg[v + 1]);
  const int hi = e < lo + ES_CHUNK ? e : lo + ES_CHUNK;
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.f;
  es_sum_hits<VEC>(dy, order, lo, hi, H, c0, lane, a);
  float* dst = part + (int64_t)(k - 1) * H;
  if (VEC) {
    const int c = c0 + lane * 8;
    if (c < H) {
      *reinterpret_cast<f32x4*>(dst + c) = f32x4{a[0], a[1], a[2], a[3]};
      *reinterpret_cast<f32x4*>(dst + c + 4) = f32x4{a[4], a[5], a[6], a[7]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j * WAVE + lane;
      if (c < H) dst[c] = a[j];
    }
  }
}

// Round the lane's accumulators once and store its columns of step c0.
template <bool VEC>
__device__ __forceinline__ void es_store_row(short* __restrict__ dst, int H,
                                             int c0, int lane,
                                             const float (&a)[8]) {
  if (VEC) {
    const int c = c0 + lane * 8;
    if (c < H) {
      s16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(a[j]);
      *reinterpret_cast<s16x8*>(dst + c) = o;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j * WAVE + lane;
      if (c < H) dst[c] = f2bf(a[j]);
    }
  }
}

// Every row that no slot boundary cuts: the empty ones, which store zeros,
// and the short ones, summed here in sorted order.  A cut row belongs to
// embed_fold_kernel.
template <bool VEC>
__global__ void __launch_bounds__(256) embed_row_kernel(
    const short* __restrict__ dy, const int* __restrict__ order,
    const int* __restrict__ seg, short* __restrict__ dtable, int64_t V,
    int H) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  for (int64_t v = (int64_t)blockIdx.x * ES_WAVES + wid; v < V;
       v += (int64_t)gridDim.x * ES_WAVES) {
    const int s = __builtin_amdgcn_readfirstlane(seg[v]);
    const int e = __builtin_amdgcn_readfirstlane(seg[v + 1]);
    const int cut = (s | (ES_CHUNK - 1)) + 1;  // end of the slot s lies in
    if (cut < e) continue;
    for (int c0 = 0; c0 < H; c0 += ES_COLS) {
      float a[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = 0.f;
      es_sum_hits<VEC>(dy, order, s, e, H, c0, lane, a);
      es_store_row<VEC>(dtable + v * H, H, c0, lane, a);
    }
  }
}

// a += partial rows of the slots lo, lo + ES_CHUNK, ... below e, in that
// order, ES_INFLIGHT of them loaded before the first is added.
template <bool VEC>
__device__ __forceinline__ void es_add_partials(const float* __restrict__ part,
                                                int lo, int e, int H, int c0,
                                                int lane, float (&a)[8]) {
  if (VEC) {
    const int c = c0 + lane * 8;
    if (c >= H) return;
    const float* src = part + (int64_t)((lo >> ES_LOG2_CHUNK) - 1) * H + c;
    for (; lo + (ES_INFLIGHT - 1) * ES_CHUNK < e;
         lo += ES_INFLIGHT * ES_CHUNK, src += (int64_t)ES_INFLIGHT * H) {
      f32x4 p[ES_INFLIGHT][2];
#pragma unroll
      for (int u = 0; u < ES_INFLIGHT; ++u) {
        p[u][0] = *reinterpret_cast<const f32x4*>(src + (int64_t)u * H);
        p[u][1] = *reinterpret_cast<const f32x4*>(src + (int64_t)u * H + 4);
      }
#pragma unroll
      for (int u = 0; u < ES_INFLIGHT; ++u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] += p[u][0][j];
          a[4 + j] += p[u][1][j];
        }
      }
    }
    for (; lo < e; lo += ES_CHUNK, src += H) {
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(src);
      const f32x4 p1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] += p0[j];
        a[4 + j] += p1[j];
      }
    }
  } else {
    for (; lo < e; lo += ES_CHUNK) {
      const float* src = part + (int64_t)((lo >> ES_LOG2_CHUNK) - 1) * H;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j * WAVE + lane;
        if (c < H) a[j] += src[c];
      }
    }
  }
}

// The cut rows, one wave per (slot boundary, column step) like the chunk
// kernel: the wave at the first boundary a row crosses sums the row's head
// (the occurrences before that boundary), adds the row's partials in slot
// order and stores its column step of the row; the others have nothing to do.
template <bool VEC>
__global__ void __launch_bounds__(256) embed_fold_kernel(
    const short* __restrict__ dy, const int* __restrict__ order,
    const int* __restrict__ keys, const int* __restrict__ seg,
    const float* __restrict__ part, short* __restrict__ dtable, int H,
    int64_t V) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int c0 = ((int)blockIdx.y * ES_WAVES + wid) * ES_COLS;
  if (c0 >= H) return;
  const int lo = ((int)blockIdx.x + 1) << ES_LOG2_CHUNK;
  const int v = __builtin_amdgcn_readfirstlane(keys[lo]);
  if (v >= V) return;
  const int s = __builtin_amdgcn_readfirstlane(seg[v]);
  if (s >= lo || s < lo - ES_CHUNK) return;  // not cut here, or cut earlier
  const int e = __builtin_amdgcn_readfirstlane(seg[v + 1]);
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.f;
  es_sum_hits<VEC>(dy, order, s, lo, H, c0, lane, a);
  es_add_partials<VEC>(part, lo, e, H, c0, lane, a);
  es_store_row<VEC>(dtable + (int64_t)v * H, H, c0, lane, a);
}

extern "C" {
int64_t embed_bwd_sorted_scratch(int64_t N, int64_t V) {
  const EsPlan p = es_plan(N, V);
  return 4 * N + ((int64_t)p.blocks * ES_WAVES << ES_MAX_DBITS) + V + 1;
}

int64_t embed_bwd_sorted_partials(int64_t N) {
  const int64_t slots = (N + ES_CHUNK - 1) / ES_CHUNK;
  return slots > 1 ? slots - 1 : 0;
}

void embed_bwd_sorted_launch(const void* dy, const int64_t* ids, int* scratch,
                             float* partials, void* dtable, int64_t N, int H,
                             int64_t V, hipStream_t s) {
  static_assert((ES_MAX_BLOCKS * ES_WAVES << ES_MAX_DBITS) <=
                    ES_SCAN_THREADS * 128, "scan entries per thread");
  const EsPlan p = es_plan(N, V);
  const int nw = p.blocks * ES_WAVES;
  int* keys[2] = {scratch, scratch + 2 * N};
  int* pos[2] = {scratch + N, scratch + 3 * N};
  int* hist = scratch + 4 * N;
  int* seg = hist + ((int64_t)nw << ES_MAX_DBITS);
  const int keymask = (int)(((int64_t)1 << p.bits) - 1);
  const dim3 grid(p.blocks);
  int shift = 0;
  for (int pass = 0; pass < p.npass; ++pass) {
    // the remaining bits spread evenly over the remaining passes
    const int dbits = (p.bits - shift + p.npass - pass - 1) / (p.npass - pass);
    const int* kin = keys[(pass + 1) & 1];
    const int* pin = pos[(pass + 1) & 1];
    int* kout = keys[pass & 1];
    int* pout = pos[pass & 1];
    if (pass == 0)
      hipLaunchKernelGGL(embed_sort_hist_kernel<true>, grid, dim3(256), 0, s,
                         ids, kin, hist, N, p.span, shift, dbits, keymask, V);
    else
      hipLaunchKernelGGL(embed_sort_hist_kernel<false>, grid, dim3(256), 0, s,
                         ids, kin, hist, N, p.span, shift, dbits, keymask, V);
    hipLaunchKernelGGL(embed_sort_scan_kernel, dim3(1), dim3(ES_SCAN_THREADS),
                       0, s, hist, nw << dbits);
    if (pass == 0)
      hipLaunchKernelGGL(embed_sort_rank_kernel<true>, grid, dim3(256), 0, s,
                         ids, kin, pin, (const int*)hist, kout, pout, N,
                         p.span, shift, dbits, keymask, V);
    else
      hipLaunchKernelGGL(embed_sort_rank_kernel<false>, grid, dim3(256), 0, s,
                         ids, kin, pin, (const int*)hist, kout, pout, N,
                         p.span, shift, dbits, keymask, V);
    shift += dbits;
  }
  const int* skeys = keys[(p.npass - 1) & 1];
  const int* order = pos[(p.npass - 1) & 1];
  hipLaunchKernelGGL(embed_seg_kernel, dim3((unsigned)((V + 256) / 256)),
                     dim3(256), 0, s, skeys, seg, (int)N, V);
  const bool vec = (H & 7) == 0 && ((uintptr_t)dy & 15) == 0;
  const int64_t nparts = embed_bwd_sorted_partials(N);
  if (nparts > 0) {
    const int csteps = (H + ES_COLS - 1) / ES_COLS;
    const dim3 cgrid((unsigned)nparts, (csteps + ES_WAVES - 1) / ES_WAVES);
    if (vec) {
      hipLaunchKernelGGL(embed_chunk_kernel<true>, cgrid, dim3(256), 0, s,
                         (const short*)dy, order, skeys, (const int*)seg,
                         partials, H, V);
      hipLaunchKernelGGL(embed_fold_kernel<true>, cgrid, dim3(256), 0, s,
                         (const short*)dy, order, skeys, (const int*)seg,
                         (const float*)partials, (short*)dtable, H, V);
    } else {
      hipLaunchKernelGGL(embed_chunk_kernel<false>, cgrid, dim3(256), 0, s,
                         (const short*)dy, order, skeys, (const int*)seg,
                         partials, H, V);
      hipLaunchKernelGGL(embed_fold_kernel<false>, cgrid, dim3(256), 0, s,
                         (const short*)dy, order, skeys, (const int*)seg,
                         (const float*)partials, (short*)dtable, H, V);
    }
  }
  const int64_t want = (V + ES_WAVES - 1) / ES_WAVES;
  const dim3 rgrid((unsigned)(want < ES_ROW_GRID_CAP ? want : ES_ROW_GRID_CAP));
  if (vec)
    hipLaunchKernelGGL(embed_row_kernel<true>, rgrid, dim3(256), 0, s,
                       (const short*)dy, order, (const int*)seg,
                       (short*)dtable, V, H);
  else
    hipLaunchKernelGGL(embed_row_kernel<false>, rgrid, dim3(256), 0, s,
                       (const short*)dy, order, (const int*)seg,
                       (short*)dtable, V, H);
}
}
