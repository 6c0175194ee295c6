// Device code shared by attention_fwd.hip and attention_bwd.hip: the tile
// constants, the MFMA wrapper, the LDS-DMA staging of a pair of tiles, the
// XCD-aware block remap, and the q-row groups and document window of the
// forward / dq blocks.
// The fragment-order helpers (perm16, cpos16, st_idx, tr16_frag_st,
// cvt_pk_bf16) are in common.h.
#pragma once
#include "common.h"

using bf16x8 = s16x8;

constexpr int QBLK = 128;  // q rows per forward / dq block (32 per wave)
constexpr int KVBLK = 64;  // rows of one staged LDS tile
#define LOG2E 1.4426950408889634f

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Stages rows [row0, row0 + 64) of two [S][stride] bf16 tensors (D columns
// from ga / gb) into the LDS tiles la / lb as st_idx images, by LDS-DMA
// (global_load_lds): no staging registers, no ds_write pass, no vmcnt park.
// 256 threads; every wave issues D/32 chunks per tensor.
//
// One wave-instruction lands 1 KiB at lds_base + lane*16 with per-lane
// global sources (probed: tools/gldsprobe.hip).  Chunk ch is half a 16-col
// subtile: lane l sources row (ch&1)*32 + l/2, cols (ch>>1)*16 + (l&1)*8,
// so the contiguous landing at tile + ch*512 is exactly st_idx(row, col).
// Rows past S-1 re-read row S-1 (in bounds; the kernels mask them).
//
// The LDS base must stay provably wave-uniform — the tile base plus a
// multiple of wid and the unrolled i, nothing lane-derived — or the
// compiler silently falls back to load + ds_write (fewer global_load_lds
// in the ISA; _hip/README.md).  Callers issue this a full tile ahead, into
// the buffer the current tile does not read.
template <int D>
__device__ __forceinline__ void stage_tile_pair(
    const short* ga, const short* gb, int64_t stride, int row0, int S,
    short* la, short* lb, int wid, int lane) {
  constexpr int ncw = D >> 5;  // chunks per wave per tensor
#pragma unroll
  for (int i = 0; i < ncw; ++i) {
    const int ch = wid * ncw + i;
    int row = row0 + (ch & 1) * 32 + (lane >> 1);
    if (row >= S) row = S - 1;
    const int64_t goff =
        (int64_t)row * stride + (ch >> 1) * 16 + (lane & 1) * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(ga + goff),
        (LDS_AS unsigned int*)(la + ch * 512), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(gb + goff),
        (LDS_AS unsigned int*)(lb + ch * 512), 16, 0, 0);
  }
}

// XCD-aware block remap (guide T1): the dispatcher places block i on XCD
// i%8, so when the ngroups = B*Hkv (batch, kv-head) groups divide over the
// 8 XCDs, the bpg blocks of one group are dealt to one XCD and the group's
// K/V (dkdv: Q/dO too) stay in that XCD's L2.  Performance only: either
// branch is a bijection of the grid.
struct GroupBlock {
  int gid;     // (batch, kv-head) group, b * Hkv + hkv
  int within;  // block within its group, 0 .. bpg-1
};
__device__ __forceinline__ GroupBlock xcd_remap(int bid, int ngroups,
                                                int bpg) {
  if ((ngroups & 7) == 0)
    return {(bid >> 3) / bpg * 8 + (bid & 7), (bid >> 3) % bpg};
  return {bid / bpg, bid % bpg};
}

// A forward / dq wave's 32 q rows are two 16-row groups INTERLEAVED across
// the block (rows w*16 and w*16+64 of the q tile at q0): every wave then
// touches both halves of the q range, so causal tile-skipping is uniform
// across waves and no wave idles at the per-tile barrier.  First row of
// group nq:
__device__ __forceinline__ int qgroup_row(int q0, int wid, int nq) {
  return q0 + nq * 64 + wid * 16;
}

// Document window of a forward / dq block.  doc_start [B,S] holds, per
// token, the first token of its document, and is monotone along a row.
//   dstart[nq]  per lane: first visible key of q row qgroup_row(nq) + l15
//               (clamped like the row itself)
//   dsmax[nq]   largest dstart of 16-row group nq (its last valid row): the
//               wave-uniform "this tile needs a mask" test
//   returns t0  first K/V tile of the block: no row of the q tile sees a
//               key before its first row's document
// All zero without DOC.  (Plain arrays, not a struct: with a struct the
// compiler schedules dq<64, DOC> differently.)
template <bool DOC>
__device__ __forceinline__ int doc_window(const int* doc_start, int b, int S,
                                          int q0, int wid, int l15,
                                          int (&dstart)[2], int (&dsmax)[2]) {
  dstart[0] = dstart[1] = dsmax[0] = dsmax[1] = 0;
  if (!DOC) return 0;
  const int* dsb = doc_start + (int64_t)b * S;
#pragma unroll
  for (int nq = 0; nq < 2; ++nq) {
    dstart[nq] = dsb[min(qgroup_row(q0, wid, nq) + l15, S - 1)];
    dsmax[nq] = dsb[min(qgroup_row(q0, wid, nq) + 15, S - 1)];
  }
  // clamped to the contract (0 <= doc_start[i] <= i) so that a bad table
  // cannot move the staging loads out of bounds
  return min(max(dsb[q0], 0), q0) / KVBLK;
}

// LDS buffer of tile t in a double-buffered loop that starts at tile t0
// with the prologue staging t0 into buffer 0: the index counts from t0, not
// from tile 0 — with `t & 1` an odd t0 computes on the buffer the prologue
// did not fill.
__device__ __forceinline__ int tile_buf(int t, int t0) { return (t - t0) & 1; }
