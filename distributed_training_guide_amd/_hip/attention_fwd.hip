// Causal flash-attention forward for gfx950: swapped-operand S^T MFMA with
// in-register P, double-buffered LDS K/V tiles DMA-staged a full tile ahead,
// one barrier per tile.
//
// Replaces the reference's flash-attn-2 dependency
// (attn_implementation="flash_attention_2", 05:93 / 06:73 / 07:71 —
// SURVEY.md §2b "Flash attention 2").
//
// Layout: q [B,S,Hq,D], k/v [B,S,Hkv,D] bf16 contiguous (BSHD). GQA via
// Hq % Hkv == 0. Causal always; the DOC instantiation additionally confines
// each query to its own document of a packed row (flash-attn-2's varlen
// masking). Saves lse [B,Hq,S] f32 for the backward.
//
// Design (guide §5.5 / §5 "common mistakes"):
//   * S^T = mfma(A=K, B=Q): the C fragment then holds qrow = lane&15 —
//     softmax rows are (mostly) lane-local: 16 values in registers + two
//     shfl_xor steps, instead of 16-lane tree reductions per row.
//   * Key-permuted A fragments (perm16): K rows are fed to the QK^T MFMA in
//     an order chosen so the C-fragment's per-lane key positions (cpos16)
//     equal the B-operand layout that P^T needs for the P·V MFMA. P
//     therefore never leaves registers: exp -> v_cvt_pk_bf16_f32 -> B
//     fragment. No P LDS round-trip, no block barrier between QK^T and P·V.
//   * K and V tiles are both ROW-major st_idx images (16-col subtiles) in
//     double-buffered LDS, landed by LDS-DMA (stage_tile_pair) with tile
//     t+1 issued at the TOP of tile t's compute: the ~200-900cy global
//     latency lands behind a full tile of MFMA (T14; PMC before: 67%
//     SQ_WAIT_ANY on the direct-global K path). One barrier per KV tile
//     (ping-pong buffers).
//   * K A-fragments are b128 row reads of that image (~50cy, interleaved
//     with the MFMA stream by the compiler); V^T A-fragments — 8
//     consecutive keys per lane — come from the same kind of image through
//     the tr16 hardware-transpose read (tr16_frag_st): no transposed copy.
//   * The XCD-aware remap (xcd_remap) keeps a (b,kv-head) group's K/V on
//     one XCD's L2.
//   * O^T accumulates in C fragments (qrow = lane&15 throughout); the
//     softmax is one fma (scale*log2(e) as its multiplier) and one raw
//     v_exp_f32 (__builtin_amdgcn_exp2f) per score; the epilogue writes 4
//     consecutive d per lane (b64).
//
// MFMA fragment maps (gfx950 v_mfma_f32_16x16x32_bf16):
//   A[m][k]: lane l holds m = l&15, k = (l>>4)*8 + j (j=0..7)
//   B[k][n]: lane l holds n = l&15, k = (l>>4)*8 + j
//   C/D     : lane l holds n = l&15, m = (l>>4)*4 + r (r=0..3)
#include "attention_common.h"
#include "launchers.h"

// DOC adds the intra-document mask of packed rows: doc_start [B,S] int32
// holds, per token, the index of the first token of its document; query i
// sees key j iff doc_start[b,i] <= j <= i.  DOC=false is the plain causal
// kernel (doc_start unused, may be null).
//
// The head dim D is a template parameter (64 or 128): with a run-time D
// every kc/dt step of the tile loop carried its own `if (kc < nkc)` branch,
// which split the MFMA stream into one basic block per step (a full LDS
// wait before every 4 MFMAs, no hoisting of operand reads across steps).
template <int D, bool DOC>
__global__ void __launch_bounds__(256, 2) attn_fwd_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse_out, int B, int S, int Hq, int Hkv, float scale,
    const int* __restrict__ doc_start) {
  static_assert(D == 64 || D == 128, "head dim must be 64 or 128");
  // both tiles in the 16-col-subtile image (st_idx; conflict-free tr16
  // reads + b128 row reads), double-buffered
  __shared__ short k_lds[2][KVBLK * D];
  __shared__ short v_lds[2][KVBLK * D];

  const int ntq = (S + QBLK - 1) / QBLK;
  const int gqa = Hq / Hkv;
  const int bpg = gqa * ntq;  // blocks per (b, hkv) group

  const GroupBlock gb = xcd_remap(blockIdx.x, B * Hkv, bpg);
  const int b = gb.gid / Hkv;
  const int hkv = gb.gid % Hkv;
  const int h = hkv * gqa + gb.within / ntq;
  const int qtile = gb.within % ntq;

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  // this wave's 32 q rows: two interleaved 16-row groups (qgroup_row)
  const int q0 = qtile * QBLK;
  const int rowb[2] = {qgroup_row(q0, wid, 0), qgroup_row(q0, wid, 1)};
  constexpr int nd16 = D >> 4;             // 16-d tiles (8 for D=128)
  constexpr int nkc = D >> 5;              // 32-d MFMA K chunks
  const int64_t strideS_q = (int64_t)Hq * D;
  const int64_t strideS_kv = (int64_t)Hkv * D;
  const short* qb = q + ((int64_t)b * S * Hq + h) * D;
  const short* kb = k + ((int64_t)b * S * Hkv + hkv) * D;
  const short* vb = v + ((int64_t)b * S * Hkv + hkv) * D;

  // ---- Q B-fragments: [nq 2][kc], row q0 + nq*16 + l15, d = kc*32+lg*8 --
  bf16x8 qf[2][nkc];
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
    int qrow = rowb[nq] + l15;
    if (qrow >= S) qrow = S - 1;
    const short* qp = qb + (int64_t)qrow * strideS_q + lg * 8;
#pragma unroll
    for (int kc = 0; kc < nkc; ++kc)
      qf[nq][kc] = *reinterpret_cast<const bf16x8*>(qp + kc * 32);
  }

  // A-fragment row l15 of tile mt carries key perm16(mt, l15), so the packed
  // P rows are already in the P·V MFMA's B-operand key order; cpos16 is the
  // matching first key of this lane's C positions (for the masks).
  // Computed once here: with the calls inside the tile loop the compiler
  // spends 4-12 more VGPRs on this kernel.
  int kperm[4], ckey[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    kperm[mt] = perm16(mt, l15);
    ckey[mt] = cpos16(mt, lg);
  }

  // O^T accumulators: [d tile][nq] C frags; lane: qrow=l15, d=lg*4+r
  f32x4 oacc[nd16][2];
#pragma unroll
  for (int dt = 0; dt < nd16; ++dt)
#pragma unroll
    for (int nq = 0; nq < 2; ++nq) oacc[dt][nq] = {0.f, 0.f, 0.f, 0.f};
  // running row max, raw (for lse) and pre-multiplied by scale*log2(e)
  // (the exponent offset of everything accumulated so far)
  float mrow[2] = {-INFINITY, -INFINITY};
  float mcrow[2] = {-INFINITY, -INFINITY};
  float lrow[2] = {0.f, 0.f};

  const int kv_end = min(S, q0 + QBLK);
  const int ntiles = (kv_end + KVBLK - 1) / KVBLK;
  const float c = scale * LOG2E;
  int dstart[2], dsmax[2];
  const int t0 =
      doc_window<DOC>(doc_start, b, S, q0, wid, l15, dstart, dsmax);

  // tile t+1's DMA issues at the top of tile t and completes under a full
  // tile of MFMA before the end-of-tile barrier
  auto stage_kv = [&](int t, int buf) {
    stage_tile_pair<D>(kb, vb, strideS_kv, t * KVBLK, S, k_lds[buf],
                       v_lds[buf], wid, lane);
  };
  stage_kv(t0, 0);
  __syncthreads();

  for (int t = t0; t < ntiles; ++t) {
    const int kv0 = t * KVBLK;
    const int buf = tile_buf(t, t0);
    if (t + 1 < ntiles) stage_kv(t + 1, buf ^ 1);

    // Both 16-row groups are computed unconditionally on every tile: an
    // `if (act0)`-guarded MFMA accumulation (skipping group 0 on its
    // fully-masked diagonal tiles) miscompiled in the dq kernel of
    // attention_bwd.hip (sparse wrong accumulator values; hipcc/ROCm 7.2)
    // — the causal mask yields p=0 / alpha=1 there, so skipping is a
    // ~3% optimization not worth the hazard.

    // ---- S^T = mfma(K, Q): [mt 4][nq 2] C frags; K A-frags from the
    // row-major staged tile (ds_read_b128, ~50cyc, hidden by MFMA) ----
    const short* kl = k_lds[buf];
    f32x4 sfrag[4][2];
    __builtin_amdgcn_s_setprio(1);  // T5: prioritize the QK^T MFMA stream
#pragma unroll
    for (int mth = 0; mth < 2; ++mth) {
      // two key-tiles at once -> 4 independent accumulator chains (the
      // dependent-accumulator MFMA latency exceeds the issue rate; a
      // 2-chain version left the pipe half idle)
      const int kra = kperm[2 * mth], krb = kperm[2 * mth + 1];
      f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
      f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < nkc; ++kc) {
        bf16x8 kfa = *reinterpret_cast<const bf16x8*>(
            kl + st_idx(kra, kc * 32 + lg * 8));
        bf16x8 kfb = *reinterpret_cast<const bf16x8*>(
            kl + st_idx(krb, kc * 32 + lg * 8));
        a0 = mfma16(kfa, qf[0][kc], a0);
        b0 = mfma16(kfb, qf[0][kc], b0);
        a1 = mfma16(kfa, qf[1][kc], a1);
        b1 = mfma16(kfb, qf[1][kc], b1);
      }
      sfrag[2 * mth][0] = a0;
      sfrag[2 * mth][1] = a1;
      sfrag[2 * mth + 1][0] = b0;
      sfrag[2 * mth + 1][1] = b1;
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- causal mask + online softmax (rows lane-local) ----
    // p = exp2(s*c - m*c) as one fma and one raw v_exp_f32 per score.
    // Masked scores are -inf (set only on tiles that need a mask) and
    // exp2(-inf) = 0 without a per-score guard, provided the offset is
    // finite: a row with no visible key yet has m = -inf, and takes a
    // finite stand-in for m*c — once per row, not once per score.
    u32x4 pk[2][2];  // [nq][kc]: 4 regs of 2 bf16 (keys j=0..7)
    float alpha[2];
#pragma unroll
    for (int nq = 0; nq < 2; ++nq) {
      const int qrow = rowb[nq] + l15;
      const bool need_mask = (kv0 + KVBLK - 1) > rowb[nq] ||
                             kv_end < kv0 + KVBLK ||
                             (DOC && dsmax[nq] > kv0);
      if (need_mask) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int key = kv0 + ckey[mt] + r;
            if (key > qrow || key >= S || (DOC && key < dstart[nq]))
              sfrag[mt][nq][r] = -INFINITY;
          }
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        f32x4 s = sfrag[mt][nq];
        tmax = fmaxf(tmax, fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])));
      }
      // row spread over lanes l15, l15+16, l15+32, l15+48
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, WAVE));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
      const float mnew = fmaxf(mrow[nq], tmax);
      const float mcn = mnew * c;
      const float mc = (mnew == -INFINITY) ? 0.0f : mcn;
      // first visible tile of a row: mcrow = -inf gives alpha = 0
      alpha[nq] = __builtin_amdgcn_exp2f(mcrow[nq] - mc);
      mrow[nq] = mnew;
      mcrow[nq] = mcn;
      float psum = 0.f;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        f32x4 s = sfrag[mt][nq];
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c, -mc));
          psum += p[r];
        }
        // keys of this C tile are already in B-operand order: mt -> (kc =
        // mt>>1, reg pair = (mt&1)*2 + {0,1})
        pk[nq][mt >> 1][(mt & 1) * 2 + 0] = cvt_pk_bf16(p[0], p[1]);
        pk[nq][mt >> 1][(mt & 1) * 2 + 1] = cvt_pk_bf16(p[2], p[3]);
      }
      psum += __shfl_xor(psum, 16, WAVE);
      psum += __shfl_xor(psum, 32, WAVE);
      lrow[nq] = lrow[nq] * alpha[nq] + psum;
    }

    // ---- O^T += mfma(V^T, P^T): V^T A-frags via tr16 hardware-transpose
    // reads from the row-major V tile (no transposed copy) ----
    const short* vt = v_lds[buf];
    __builtin_amdgcn_s_setprio(1);  // T5: prioritize the P.V MFMA stream
#pragma unroll
    for (int dt = 0; dt < nd16; ++dt) {
      bf16x8 va[2];
#pragma unroll
      for (int kc = 0; kc < 2; ++kc)
        va[kc] = tr16_frag_st(vt, kc * 32 + lg * 8, dt * 16, l15);
#pragma unroll
      for (int nq = 0; nq < 2; ++nq) {
        f32x4 acc = oacc[dt][nq];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= alpha[nq];
        acc = mfma16(va[0], __builtin_bit_cast(bf16x8, pk[nq][0]), acc);
        acc = mfma16(va[1], __builtin_bit_cast(bf16x8, pk[nq][1]), acc);
        oacc[dt][nq] = acc;
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }

  // ---- epilogue: lane holds qrow = l15, d = dt*16 + lg*4 + r ----
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
    const int qrow = rowb[nq] + l15;
    if (qrow >= S) continue;
    const float invl = (lrow[nq] > 0.f) ? 1.0f / lrow[nq] : 0.0f;
    short* op = o + ((int64_t)b * S * Hq + (int64_t)qrow * Hq + h) * D;
#pragma unroll
    for (int dt = 0; dt < nd16; ++dt) {
      s16x4 outv;
#pragma unroll
      for (int r = 0; r < 4; ++r) outv[r] = f2bf(oacc[dt][nq][r] * invl);
      *reinterpret_cast<s16x4*>(op + dt * 16 + lg * 4) = outv;
    }
    if (lg == 0)
      lse_out[((int64_t)b * Hq + h) * S + qrow] =
          mrow[nq] * scale + __logf(fmaxf(lrow[nq], 1e-30f));
  }
}

extern "C" void attn_fwd_launch(const void* q, const void* k, const void* v,
                                void* o, float* lse, const int* doc_start,
                                int B, int S, int Hq, int Hkv, int D,
                                float scale, hipStream_t stream) {
  int ntiles = (S + QBLK - 1) / QBLK;
  int64_t grid = (int64_t)B * Hq * ntiles;
  // bindings.cpp admits D of 64 or 128 only
  auto kern = doc_start
                  ? (D == 64 ? attn_fwd_kernel<64, true>
                             : attn_fwd_kernel<128, true>)
                  : (D == 64 ? attn_fwd_kernel<64, false>
                             : attn_fwd_kernel<128, false>);
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(256), 0, stream,
                     (const short*)q, (const short*)k, (const short*)v,
                     (short*)o, lse, B, S, Hq, Hkv, scale, doc_start);
}
