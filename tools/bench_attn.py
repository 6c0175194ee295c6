#!/usr/bin/env python3
"""Micro-benchmark for the attention kernels (run on a GPU box).

Reports achieved TFLOP/s for forward and backward at training shapes,
causal-masked FLOP accounting (guide §5.4: random data, within-run timing).

--docs N runs the document-masked kernels instead, on rows of N equal-length
documents, and reports TF/s under two accountings: causal-equivalent (the
FLOPs the plain causal kernel would spend on the row) and the query/key pairs
the mask actually leaves visible.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--B", type=int, default=8)
    p.add_argument("--S", type=int, default=1024)
    p.add_argument("--Hq", type=int, default=32)
    p.add_argument("--Hkv", type=int, default=8)
    p.add_argument("--D", type=int, default=128)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--check", action="store_true")
    p.add_argument("--docs", type=int, default=0,
                   help="N equal-length documents per row through the "
                        "doc-masked kernels (0 = plain causal kernels)")
    args = p.parse_args()
    if args.docs:
        return bench_docs(args)

    from distributed_training_guide_amd._ext import ext
    from distributed_training_guide_amd.ops import reference as R

    torch.manual_seed(0)
    B, S, Hq, Hkv, D = args.B, args.S, args.Hq, args.Hkv, args.D
    q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
    scale = D ** -0.5

    # causal flop accounting: 2 gemms fwd, 5 gemms bwd, x0.5 causal
    flops_fwd = 4 * B * Hq * S * S * D * 0.5
    flops_bwd = 10 * B * Hq * S * S * D * 0.5

    o, lse = ext().attn_fwd(q, k, v, scale)
    if args.check:
        orf = R.attention_ref(q.float(), k.float(), v.float(), scale)
        err = (o.float() - orf).norm() / orf.norm()
        print(f"fwd rel err: {err.item():.4f}")
        assert err < 3e-2

    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.iters):
        o, lse = ext().attn_fwd(q, k, v, scale)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / args.iters
    print(f"fwd: {dt * 1e3:.3f} ms  {flops_fwd / dt / 1e12:.1f} TF/s")

    do = torch.randn_like(o)
    dq, dk, dv = ext().attn_bwd(do, q, k, v, o, lse, scale)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.iters):
        dq, dk, dv = ext().attn_bwd(do, q, k, v, o, lse, scale)
    torch.cuda.synchronize()
    dt = (time.time() - t0) / args.iters
    print(f"bwd: {dt * 1e3:.3f} ms  {flops_bwd / dt / 1e12:.1f} TF/s")


def visited_tiles(S, L):
    """K/V tiles the forward (= dq) and q tiles the dk/dv kernel visit per
    (batch row, head) for documents of length L, and for plain causal."""
    fwd = fwd_c = 0
    for qt in range((S + 127) // 128):
        ntiles = (min(S, qt * 128 + 128) + 63) // 64
        fwd_c += ntiles
        fwd += ntiles - (qt * 128 // L * L) // 64
    dkdv = dkdv_c = 0
    for kt in range((S + 63) // 64):
        last = min(kt * 64 + 63, S - 1)
        dkdv_c += (S - kt * 64 + 63) // 64
        dkdv += (min(S, (last // L + 1) * L) - kt * 64 + 63) // 64
    return dict(fwd=fwd, fwd_causal=fwd_c, dkdv=dkdv, dkdv_causal=dkdv_c)


def bench_docs(args):
    from distributed_training_guide_amd._ext import ext
    from distributed_training_guide_amd.ops import doc_bounds
    from distributed_training_guide_amd.ops import reference as R

    torch.manual_seed(0)
    B, S, Hq, Hkv, D, N = args.B, args.S, args.Hq, args.Hkv, args.D, args.docs
    if S % N:
        raise SystemExit("--docs must divide --S")
    L = S // N
    q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
    scale = D ** -0.5
    idx = torch.arange(S, device="cuda", dtype=torch.int32)
    doc = doc_bounds((idx // L * L).repeat(B, 1))

    pairs_causal = S * S * 0.5
    pairs_visible = N * L * L * 0.5
    tiles = visited_tiles(S, L)
    print(f"docs: {N} x {L} tokens; visible/causal pairs "
          f"{pairs_visible / pairs_causal:.4f}; tiles fwd/dq "
          f"{tiles['fwd']}/{tiles['fwd_causal']} dkdv "
          f"{tiles['dkdv']}/{tiles['dkdv_causal']}")

    o, lse = ext().attn_fwd_doc(q, k, v, doc.start, scale)
    if args.check:
        orf = R.attention_ref(q.float(), k.float(), v.float(), scale,
                              doc_start=doc.start)
        err = (o.float() - orf).norm() / orf.norm()
        print(f"fwd rel err: {err.item():.4f}")
        assert err < 3e-2

    def report(name, dt, gemms):
        eq = gemms * 2 * B * Hq * D * pairs_causal / dt / 1e12
        vis = gemms * 2 * B * Hq * D * pairs_visible / dt / 1e12
        print(f"{name}: {dt * 1e3:.3f} ms  {eq:.1f} TF/s causal-equivalent  "
              f"{vis:.1f} TF/s visible-pairs")

    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.iters):
        o, lse = ext().attn_fwd_doc(q, k, v, doc.start, scale)
    torch.cuda.synchronize()
    report("fwd", (time.time() - t0) / args.iters, 2)

    do = torch.randn_like(o)
    bwd = lambda: ext().attn_bwd_doc(do, q, k, v, o, lse, doc.start, doc.end,
                                     scale)
    bwd()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(args.iters):
        bwd()
    torch.cuda.synchronize()
    report("bwd", (time.time() - t0) / args.iters, 5)


if __name__ == "__main__":
    main()
