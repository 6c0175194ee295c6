// Causal flash-attention backward for gfx950, the counterpart of
// attention_fwd.hip with the same idiom set: swapped / permuted MFMA
// fragments with P and dS packed in registers, row-major st_idx tiles in
// double-buffered LDS DMA-staged a tile ahead, read as b128 rows and through
// the tr16 hardware transpose. Replaces flash-attn-2's backward
// (SURVEY.md §2b "Flash attention 2", "bwd recompute variant").
//
// Standard flash-2 backward with lse recompute, split into three atomic-free
// kernels (the loop order that would fuse them needs cross-block atomics on
// dq — prohibitive write amplification at training shapes):
//   1. delta[b,h,s] = rowsum(dO * O)
//   2. dk/dv: block owns 64 keys of one (b, hkv) (one wave = 16 keys, its
//      K/V B-fragments loaded once from global); loops (gqa-head, 64-q-row
//      tile), accumulating dK/dV in registers. The Q and dO tiles are staged
//      row-major (stage_tile_pair) and serve both the S/dP MFMAs'
//      A-fragments (b128 row reads in perm16 order) and the dV/dK MFMAs'
//      B-fragments (tr16 transpose reads); P^T/dS^T stay in registers via
//      the perm16 trick.
//   3. dq: block owns 128 q rows of one (b, hq) (one wave = 32, its Q/dO
//      B-fragments loaded once from global); loops 64-key tiles like the
//      forward, with K and V staged row-major: K serves the S^T A-fragments
//      (b128) and the dQ B-fragments (tr16), V the dP^T A-fragments; dS is
//      packed in registers as the dQ MFMA's A operand.
// Math (S_raw = Q.K^T, P = exp(scale*S_raw - lse)):
//   dV += P^T dO
//   dP = dO V^T;  dS_raw = scale * P * (dP - delta)
//   dK += dS_raw^T Q;  dQ += dS_raw K
//
// Fragment maps as in attention_fwd.hip:
//   A[m][k]: lane l -> m = l&15, k = (l>>4)*8 + j   (k spans 0..31)
//   B[k][n]: lane l -> n = l&15, k = (l>>4)*8 + j
//   C/D    : lane l -> n = l&15, m = (l>>4)*4 + r
#include "attention_common.h"
#include "launchers.h"

// ---------------- delta = rowsum(dO * O) ----------------
// one row per 16-lane group (16 lanes x 8 bf16 = 128 elems = a whole
// D=128 row per pass) — a row-per-wave version left 48/64 lanes idle at
// D<=128 (guide §5 mistake 6)
template <int D>
__global__ void __launch_bounds__(256) attn_delta_kernel(
    const short* __restrict__ dout, const short* __restrict__ o,
    float* __restrict__ delta, int B, int S, int Hq) {
  const int grp = threadIdx.x >> 4;       // 16 groups per block
  const int gl = threadIdx.x & 15;
  int64_t nrows = (int64_t)B * S * Hq;
  for (int64_t row = (int64_t)blockIdx.x * 16 + grp; row < nrows;
       row += (int64_t)gridDim.x * 16) {
    const short* dp = dout + row * D;
    const short* op = o + row * D;
    float s = 0.f;
#pragma unroll
    for (int i = gl * 8; i < D; i += 16 * 8) {
      bf16x8 dv = *reinterpret_cast<const bf16x8*>(dp + i);
      bf16x8 ov = *reinterpret_cast<const bf16x8*>(op + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += bf2f(dv[j]) * bf2f(ov[j]);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, WAVE);
    if (gl == 0) {
      // row = (b*S + s_pos)*Hq + h  ->  delta is [B, Hq, S]
      int h = (int)(row % Hq);
      int64_t bs = row / Hq;
      int sp = (int)(bs % S);
      int b = (int)(bs / S);
      delta[((int64_t)b * Hq + h) * S + sp] = s;
    }
  }
}

// ---------------- dk / dv ----------------
// DOC (both kernels below) adds the intra-document mask of packed rows; see
// attention_fwd.hip.  Each kernel reads the table that is lane-local in its
// fragment layout: dkdv owns keys, so it reads doc_end [B,S] int32 (the
// exclusive end of each key's document; q row i sees key j iff
// j <= i < doc_end[b,j]); dq owns q rows and reads doc_start like the
// forward.  DOC=false is the plain causal kernel (table unused, may be
// null).
//
// The head dim D is a template parameter (64 or 128) so that every loop
// over d-chunks has a compile-time bound (see attention_fwd.hip).  The
// per-score arithmetic is one fma + raw v_exp_f32 for P and one fma + mul
// for dS: scale*log2(e) is folded into the fma's multiplier, lse arrives
// pre-multiplied by log2(e) and delta by scale (once per row, when they
// are staged), and the causal/document mask touches only the tiles that
// need one (exp2(-inf) = 0).
template <int D, bool DOC>
__global__ void __launch_bounds__(256, 2) attn_dkdv_kernel(
    const short* __restrict__ dout, const short* __restrict__ q,
    const short* __restrict__ k, const short* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dk, short* __restrict__ dv, int B, int S, int Hq,
    int Hkv, float scale, const int* __restrict__ doc_end) {
  static_assert(D == 64 || D == 128, "head dim must be 64 or 128");
  // double-buffered ROW-major staging of the 64-q-row tile (q[qrow][d],
  // dO[qrow][d], st_idx subtile image): serves BOTH the Q/dO A-fragments
  // (b128 row reads, replacing per-tile global gathers) and the
  // dV/dK B-fragments (tr16 hardware-transpose reads); plus lse/delta rows
  __shared__ short q_lds[2][64 * D];
  __shared__ short do_lds[2][64 * D];
  __shared__ __attribute__((aligned(16))) float lse_lds[2][64];
  __shared__ __attribute__((aligned(16))) float del_lds[2][64];

  const int nkt = (S + 63) / 64;
  const int group = Hq / Hkv;

  const GroupBlock gb = xcd_remap(blockIdx.x, B * Hkv, nkt);
  const int b = gb.gid / Hkv;
  const int hkv = gb.gid % Hkv;
  const int kt = gb.within;

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int l15 = lane & 15;
  const int lg = lane >> 4;

  const int kv0 = kt * 64 + wid * 16;  // this wave's 16 keys
  constexpr int nd16 = D >> 4, nkc = D >> 5;
  const float c2 = scale * LOG2E;
  const int64_t strideS_q = (int64_t)Hq * D;
  const int64_t strideS_kv = (int64_t)Hkv * D;
  const short* kb = k + ((int64_t)b * S * Hkv + hkv) * D;
  const short* vb = v + ((int64_t)b * S * Hkv + hkv) * D;

  // K/V B-fragments (n = key l15, k = d lg*8+j — contiguous 16 B loads)
  bf16x8 kf[nkc], vf[nkc];
  {
    int key = kv0 + l15;
    int keyc = key < S ? key : S - 1;
    const short* kp = kb + (int64_t)keyc * strideS_kv + lg * 8;
    const short* vp = vb + (int64_t)keyc * strideS_kv + lg * 8;
#pragma unroll
    for (int c = 0; c < nkc; ++c) {
      kf[c] = *reinterpret_cast<const bf16x8*>(kp + c * 32);
      vf[c] = *reinterpret_cast<const bf16x8*>(vp + c * 32);
    }
  }

  // dK/dV accumulators: C[m=key][n=d] frags per d-tile
  // (lane: d = l15, key = kv0 + lg*4 + r)
  f32x4 dkacc[nd16], dvacc[nd16];
#pragma unroll
  for (int i = 0; i < nd16; ++i) {
    dkacc[i] = {0.f, 0.f, 0.f, 0.f};
    dvacc[i] = {0.f, 0.f, 0.f, 0.f};
  }

  // iteration space: (h in gqa group) x (64-row q tiles >= causal start)
  const int qstart = kt * 64;
  // DOC: this lane's key stops being visible at dend (clamped like the
  // key); dend_min is the smallest of the wave's 16 (its first key's —
  // doc_end is monotone), below which no q row needs the document test.
  // No q row at or past the end of the block's last valid key's document
  // sees any of the block's keys, so the q-tile walk stops there instead
  // of at S.
  int dend = S, dend_min = S, qcap = S;
  if (DOC) {
    const int* deb = doc_end + (int64_t)b * S;
    dend = deb[min(kv0 + l15, S - 1)];
    dend_min = deb[min(kv0, S - 1)];
    // clamped to the contract (j < doc_end[j] <= S): a bad table cannot
    // move the staging loads out of bounds
    qcap = min(max(deb[min(qstart + 63, S - 1)], qstart + 1), S);
  }
  const int nqt = (qcap - qstart + 63) / 64;
  const int niter = group * nqt;

  // the next (h, q-tile)'s Q/dO tiles stream into the other buffer one
  // iteration AHEAD, so global latency hides behind a full tile of MFMA
  auto stage_qdo = [&](int it, int buf) {
    const int64_t hoff = ((int64_t)b * S * Hq + hkv * group + it / nqt) * D;
    stage_tile_pair<D>(q + hoff, dout + hoff, strideS_q,
                       qstart + (it % nqt) * 64, S, q_lds[buf], do_lds[buf],
                       wid, lane);
  };
  // lse lands pre-multiplied by log2(e), delta by scale
  auto stage_lse = [&](int it, int buf) {
    const int hh = hkv * group + it / nqt;
    const int qt = qstart + (it % nqt) * 64;
    if (tid < 64) {
      const float* lseb = lse + ((int64_t)b * Hq + hh) * S;
      int rr = qt + tid < S ? qt + tid : S - 1;
      lse_lds[buf][tid] = lseb[rr] * LOG2E;
    } else if (tid < 128) {
      const float* delb = delta + ((int64_t)b * Hq + hh) * S;
      int rr = qt + tid - 64 < S ? qt + tid - 64 : S - 1;
      del_lds[buf][tid - 64] = delb[rr] * scale;
    }
  };

  stage_qdo(0, 0);
  stage_lse(0, 0);
  __syncthreads();

  for (int it = 0; it < niter; ++it) {
    const int buf = it & 1;
    if (it + 1 < niter) {
      stage_qdo(it + 1, buf ^ 1);
      stage_lse(it + 1, buf ^ 1);
    }

    const int qt = qstart + (it % nqt) * 64;
    const short* ql = q_lds[buf];
    const short* dol = do_lds[buf];

    // ---- per mt: S/dP MFMAs (C[m=qrow(perm)][n=key]; A = Q/dO rows in
    // perm16 order from LDS, B = kf/vf), then immediately
    // P = exp2(c2*S - lse'), dS = P*(scale*dP - delta'), packed into
    // A-operand order — only one mt of S/dP state stays live ----
    const int key = kv0 + l15;  // this lane's key (C n-position)
    // DOC also masks on every tile that reaches the end of the document
    // of the wave's first key
    const bool diag = (qt < kt * 64 + 64) || (qt + 63 >= S) ||
                      (DOC && qt + 63 >= dend_min);
    u32x4 pk_p[2], pk_ds[2];
    __builtin_amdgcn_s_setprio(1);  // T5: prioritize the MFMA stream
#pragma unroll
    for (int mth = 0; mth < 2; ++mth) {
      // two q-row tiles at once -> 4 independent MFMA accumulator chains
      // (dependent-accumulator latency > issue rate with only 2)
      const int qra = perm16(2 * mth, l15), qrb = perm16(2 * mth + 1, l15);
      f32x4 sa0 = {0.f, 0.f, 0.f, 0.f}, da0 = {0.f, 0.f, 0.f, 0.f};
      f32x4 sa1 = {0.f, 0.f, 0.f, 0.f}, da1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < nkc; ++c) {
        bf16x8 qa0 = *reinterpret_cast<const bf16x8*>(
            ql + st_idx(qra, c * 32 + lg * 8));
        bf16x8 qa1 = *reinterpret_cast<const bf16x8*>(
            ql + st_idx(qrb, c * 32 + lg * 8));
        bf16x8 do0 = *reinterpret_cast<const bf16x8*>(
            dol + st_idx(qra, c * 32 + lg * 8));
        bf16x8 do1 = *reinterpret_cast<const bf16x8*>(
            dol + st_idx(qrb, c * 32 + lg * 8));
        sa0 = mfma16(qa0, kf[c], sa0);
        sa1 = mfma16(qa1, kf[c], sa1);
        da0 = mfma16(do0, vf[c], da0);
        da1 = mfma16(do1, vf[c], da1);
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int mt = 2 * mth + half;
        const f32x4 sa = half ? sa1 : sa0;
        const f32x4 da = half ? da1 : da0;
        const int qoff = cpos16(mt, lg);
        // qoff is a multiple of 4: one b128 read each
        const f32x4 lse4 =
            *reinterpret_cast<const f32x4*>(&lse_lds[buf][qoff]);
        const f32x4 del4 =
            *reinterpret_cast<const f32x4*>(&del_lds[buf][qoff]);
        float e[4], p[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          e[r] = __builtin_fmaf(sa[r], c2, -lse4[r]);
        if (diag) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qrow = qt + qoff + r;
            if (key > qrow || qrow >= S || key >= S || (DOC && qrow >= dend))
              e[r] = -INFINITY;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[r] = __builtin_amdgcn_exp2f(e[r]);
          ds[r] = p[r] * __builtin_fmaf(da[r], scale, -del4[r]);
        }
        const int kc = mt >> 1, rp = (mt & 1) * 2;
        pk_p[kc][rp + 0] = cvt_pk_bf16(p[0], p[1]);
        pk_p[kc][rp + 1] = cvt_pk_bf16(p[2], p[3]);
        pk_ds[kc][rp + 0] = cvt_pk_bf16(ds[0], ds[1]);
        pk_ds[kc][rp + 1] = cvt_pk_bf16(ds[2], ds[3]);
      }
    }

    // ---- dV += P^T dO ; dK += dS^T Q (B operands via tr16 transpose
    // reads from the same row-major tiles) ----
#pragma unroll
    for (int dt = 0; dt < nd16; ++dt) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        bf16x8 dofr = tr16_frag_st(dol, kc * 32 + lg * 8, dt * 16, l15);
        bf16x8 qfr = tr16_frag_st(ql, kc * 32 + lg * 8, dt * 16, l15);
        dvacc[dt] = mfma16(__builtin_bit_cast(bf16x8, pk_p[kc]), dofr,
                           dvacc[dt]);
        dkacc[dt] = mfma16(__builtin_bit_cast(bf16x8, pk_ds[kc]), qfr,
                           dkacc[dt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }

  // ---- store dK/dV (exclusive: one block per (b,hkv,key)) ----
  // C layout: lane d = l15 (per dt), key = kv0 + lg*4 + r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int keyw = kv0 + lg * 4 + r;
    if (keyw >= S) continue;
    short* dkp = dk + ((int64_t)b * S * Hkv + (int64_t)keyw * Hkv + hkv) * D;
    short* dvp = dv + ((int64_t)b * S * Hkv + (int64_t)keyw * Hkv + hkv) * D;
#pragma unroll
    for (int dt = 0; dt < nd16; ++dt) {
      dkp[dt * 16 + l15] = f2bf(dkacc[dt][r]);
      dvp[dt * 16 + l15] = f2bf(dvacc[dt][r]);
    }
  }
}

// ---------------- dq ----------------
template <int D, bool DOC>
__global__ void __launch_bounds__(256, 2) attn_dq_kernel(
    const short* __restrict__ dout, const short* __restrict__ q,
    const short* __restrict__ k, const short* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dq, int B, int S, int Hq, int Hkv, float scale,
    const int* __restrict__ doc_start) {
  static_assert(D == 64 || D == 128, "head dim must be 64 or 128");
  // double-buffered K and V tiles (st_idx subtile image): K serves
  // the S^T A-fragments (b128 row reads) AND the dQ B-fragments (tr16
  // transpose reads); V serves the dP^T A-fragments
  __shared__ short k_lds[2][KVBLK * D];
  __shared__ short v_lds[2][KVBLK * D];

  const int ntq = (S + QBLK - 1) / QBLK;
  const int gqa = Hq / Hkv;
  const int bpg = gqa * ntq;

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
  constexpr int nd16 = D >> 4, nkc = D >> 5;
  const float c2 = scale * LOG2E;
  const int64_t strideS_q = (int64_t)Hq * D;
  const int64_t strideS_kv = (int64_t)Hkv * D;
  const short* qb = q + ((int64_t)b * S * Hq + h) * D;
  const short* dob = dout + ((int64_t)b * S * Hq + h) * D;
  const short* kb = k + ((int64_t)b * S * Hkv + hkv) * D;
  const short* vb = v + ((int64_t)b * S * Hkv + hkv) * D;
  const float* lseb = lse + ((int64_t)b * Hq + h) * S;
  const float* delb = delta + ((int64_t)b * Hq + h) * S;

  // Q / dO B-fragments (n = qrow = l15 per nq tile) + per-lane lse/delta,
  // lse pre-multiplied by log2(e) and delta by scale
  bf16x8 qf[2][nkc], dof[2][nkc];
  float lse_r[2], del_r[2];
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
    int qrow = rowb[nq] + l15;
    int qrc = qrow < S ? qrow : S - 1;
    const short* qp = qb + (int64_t)qrc * strideS_q + lg * 8;
    const short* dop = dob + (int64_t)qrc * strideS_q + lg * 8;
#pragma unroll
    for (int c = 0; c < nkc; ++c) {
      qf[nq][c] = *reinterpret_cast<const bf16x8*>(qp + c * 32);
      dof[nq][c] = *reinterpret_cast<const bf16x8*>(dop + c * 32);
    }
    lse_r[nq] = lseb[qrc] * LOG2E;
    del_r[nq] = delb[qrc] * scale;
  }

  // dQ accumulators: C[m=qrow][n=d] frags (lane: d = l15, qrow = lg*4+r)
  f32x4 dqacc[nd16][2];
#pragma unroll
  for (int dt = 0; dt < nd16; ++dt)
#pragma unroll
    for (int nq = 0; nq < 2; ++nq) dqacc[dt][nq] = {0.f, 0.f, 0.f, 0.f};

  const int kv_end = min(S, q0 + QBLK);
  const int ntiles = (kv_end + KVBLK - 1) / KVBLK;
  int dstart[2], dsmax[2];
  const int t0 =
      doc_window<DOC>(doc_start, b, S, q0, wid, l15, dstart, dsmax);

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

    // group 0 (lower rows) drops out at the final diagonal tiles; group 1
    // is live for every tile — uniform across waves (no barrier idling)
    // NOTE: an `if (act0)`-guarded MFMA accumulation here (skipping the
    // lower 16-row group on its fully-masked diagonal tiles) miscompiled —
    // sparse wrong dqacc[0][0] values on waves 2/3 (hipcc/ROCm 7.2, wave-
    // uniform condition derived from wid). Both groups are computed
    // unconditionally; the causal mask already zeroes dS of masked tiles.
    {
      // ---- per mt: S^T = mfma(K_perm, Q), dP^T = mfma(V_perm, dO), then
      // immediately exp/pack dS into the dQ MFMA's A operand (keys in
      // kc*32+lg*8+j order via perm16) — keeps only one mt of S/dP live ----
      const bool smask = (kv_end < kv0 + KVBLK);
      u32x4 pk_ds[2][2];  // [nq][kc]
      const short* kl = k_lds[buf];
      const short* vl = v_lds[buf];
      __builtin_amdgcn_s_setprio(1);  // T5: prioritize the MFMA stream
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int kr = perm16(mt, l15);  // local key row
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
        f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < nkc; ++c) {
          bf16x8 ka = *reinterpret_cast<const bf16x8*>(
              kl + st_idx(kr, c * 32 + lg * 8));
          bf16x8 va = *reinterpret_cast<const bf16x8*>(
              vl + st_idx(kr, c * 32 + lg * 8));
          s0 = mfma16(ka, qf[0][c], s0);
          d0 = mfma16(va, dof[0][c], d0);
          s1 = mfma16(ka, qf[1][c], s1);
          d1 = mfma16(va, dof[1][c], d1);
        }
        const int koff = cpos16(mt, lg);
        const int kc = mt >> 1, rp = (mt & 1) * 2;
#pragma unroll
        for (int nq = 0; nq < 2; ++nq) {
          const int qrow = rowb[nq] + l15;
          const bool diag = (kv0 + KVBLK - 1 > rowb[nq]) || smask ||
                            (DOC && dsmax[nq] > kv0);
          const f32x4 sv = nq ? s1 : s0;
          const f32x4 dv = nq ? d1 : d0;
          // P = exp2(c2*S - lse'), dS = P*(scale*dP - delta'); the mask
          // touches only the tiles that need one (exp2(-inf) = 0)
          float e[4], ds[4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            e[r] = __builtin_fmaf(sv[r], c2, -lse_r[nq]);
          if (diag) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int keyr = kv0 + koff + r;
              if (keyr > qrow || keyr >= S || qrow >= S ||
                  (DOC && keyr < dstart[nq]))
                e[r] = -INFINITY;
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ds[r] = __builtin_amdgcn_exp2f(e[r]) *
                    __builtin_fmaf(dv[r], scale, -del_r[nq]);
          pk_ds[nq][kc][rp + 0] = cvt_pk_bf16(ds[0], ds[1]);
          pk_ds[nq][kc][rp + 1] = cvt_pk_bf16(ds[2], ds[3]);
        }
      }

      // ---- dQ += dS K: B operand [k=key][n=d] via tr16 transpose reads
      // from the row-major K tile ----
#pragma unroll
      for (int dt = 0; dt < nd16; ++dt) {
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          bf16x8 kfr = tr16_frag_st(kl, kc * 32 + lg * 8, dt * 16, l15);
          dqacc[dt][0] = mfma16(__builtin_bit_cast(bf16x8, pk_ds[0][kc]),
                                kfr, dqacc[dt][0]);
          dqacc[dt][1] = mfma16(__builtin_bit_cast(bf16x8, pk_ds[1][kc]),
                                kfr, dqacc[dt][1]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
  }

  // ---- store dQ: lane d = l15 (per dt), qrow = q0 + nq*16 + lg*4 + r ----
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int qrow = rowb[nq] + lg * 4 + r;
      if (qrow >= S) continue;
      short* dqp = dq + ((int64_t)b * S * Hq + (int64_t)qrow * Hq + h) * D;
#pragma unroll
      for (int dt = 0; dt < nd16; ++dt) {
        dqp[dt * 16 + l15] = f2bf(dqacc[dt][nq][r]);
      }
    }
  }
}

namespace {
template <int D, bool DOC>
void bwd_launch(const short* dout, const short* q, const short* k,
                const short* v, const short* o, const float* lse,
                float* delta, short* dq, short* dk, short* dv,
                const int* doc_start, const int* doc_end, int B, int S,
                int Hq, int Hkv, float scale, hipStream_t stream) {
  int64_t nrows = (int64_t)B * S * Hq;
  int64_t dwant = (nrows + 15) / 16;
  int dgrid = (int)(dwant < 2048 ? (dwant < 1 ? 1 : dwant) : 2048);
  hipLaunchKernelGGL(attn_delta_kernel<D>, dim3(dgrid), dim3(256), 0, stream,
                     dout, o, delta, B, S, Hq);
  int nkt = (S + 63) / 64;
  hipLaunchKernelGGL((attn_dkdv_kernel<D, DOC>),
                     dim3((uint32_t)((int64_t)B * Hkv * nkt)), dim3(256), 0,
                     stream, dout, q, k, v, lse, delta, dk, dv, B, S, Hq, Hkv,
                     scale, doc_end);
  int ntq = (S + QBLK - 1) / QBLK;
  hipLaunchKernelGGL((attn_dq_kernel<D, DOC>),
                     dim3((uint32_t)((int64_t)B * Hq * ntq)), dim3(256), 0,
                     stream, dout, q, k, v, lse, delta, dq, B, S, Hq, Hkv,
                     scale, doc_start);
}
}  // namespace

extern "C" void attn_bwd_launch(const void* dout, const void* q, const void* k,
                                const void* v, const void* o, const float* lse,
                                float* delta, void* dq, void* dk, void* dv,
                                const int* doc_start, const int* doc_end,
                                int B, int S, int Hq, int Hkv, int D,
                                float scale, hipStream_t stream) {
  // bindings.cpp admits D of 64 or 128 only, and both tables or neither
  const bool doc = doc_start != nullptr;
  auto fn = doc ? (D == 64 ? bwd_launch<64, true> : bwd_launch<128, true>)
                : (D == 64 ? bwd_launch<64, false> : bwd_launch<128, false>);
  fn((const short*)dout, (const short*)q, (const short*)k, (const short*)v,
     (const short*)o, lse, delta, (short*)dq, (short*)dk, (short*)dv,
     doc_start, doc_end, B, S, Hq, Hkv, scale, stream);
}
