#!/usr/bin/env python3
"""Micro-benchmark for the fused qkv split + QK RMSNorm + RoPE kernels
(run on a GPU box).

At one attention layer's shape (default: Qwen3-8B at 24576 tokens, Hq 32,
Hkv 8, D 128) it times, alternating the variants within one process (device
events, warm-up, median / min / max of the repeats):

  fused_fwd / fused_bwd      qkv_norm_rope.hip through the raw bindings
  rope_fwd / rope_bwd        qkv_rope.hip (the same split without the norm)
  unfused_fwd / unfused_bwd  what the existing ops would take: split,
                             contiguous copies, rmsnorm on [., D] rows, rope,
                             and autograd's backward of that chain

Bytes per token: the fused forward reads and writes the packed row once,
2 * W * 2, exactly what qkv_rope's forward moves; the fused backward reads
dq/dk/dv and the saved q and k rows and writes dqkv, (3 Hq + 5 Hkv) * D * 2,
against 2 * W * 2 for qkv_rope's (136 / 96 at the default shape).

The acceptance conditions are recorded in the JSON, not preset numbers:
`fused_beats_unfused` is true when fused fwd+bwd is faster than the unfused
chain by more than the run's spread (the sum of both sides' max - min), and
`fused_fwd_slower_than_rope_fwd` when the fused forward trails qkv_rope's by
more than theirs."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=24)
    p.add_argument("--seq", type=int, default=1024)
    p.add_argument("--heads", type=int, default=32)
    p.add_argument("--kv-heads", type=int, default=8)
    p.add_argument("--head-dim", type=int, default=128)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--out", default="profiles/qk_norm.json")
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_qk_norm needs a GPU: timings are not measured on "
                 "the CPU")
    from distributed_training_guide_amd._ext import ext
    from distributed_training_guide_amd.ops import rmsnorm, rope
    from distributed_training_guide_amd.ops.rope import get_rope_tables

    C = ext()  # fail loudly without the HIP extension
    torch.manual_seed(0)
    dev = torch.device("cuda")
    B, S, Hq, Hkv, D = (args.batch, args.seq, args.heads, args.kv_heads,
                        args.head_dim)
    W = (Hq + 2 * Hkv) * D
    eps, theta = 1e-6, 1e6
    bf = dict(device=dev, dtype=torch.bfloat16)
    qkv = torch.randn(B, S, W, **bf)
    wq = (1.0 + 0.1 * torch.randn(D, device=dev)).bfloat16()
    wk = (1.0 + 0.1 * torch.randn(D, device=dev)).bfloat16()
    dq = torch.randn(B, S, Hq, D, **bf)
    dk = torch.randn(B, S, Hkv, D, **bf)
    dv = torch.randn(B, S, Hkv, D, **bf)
    cos, sin = get_rope_tables(D, S, theta, dev)

    leaf = dict(qkv=qkv.clone().requires_grad_(True),
                wq=wq.clone().requires_grad_(True),
                wk=wk.clone().requires_grad_(True))
    graph = {}

    def unfused_fwd():
        for t in leaf.values():
            t.grad = None
        q, k, v = leaf["qkv"].split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        q = rmsnorm(q.reshape(B, S, Hq, D), leaf["wq"], eps)
        k = rmsnorm(k.reshape(B, S, Hkv, D), leaf["wk"], eps)
        q = rope(q, theta, max_pos=S)
        k = rope(k, theta, max_pos=S)
        graph["out"] = (q, k, v.reshape(B, S, Hkv, D).contiguous())

    def unfused_bwd():
        torch.autograd.backward(list(graph.pop("out")), [dq, dk, dv])

    variants = {
        "fused_fwd": lambda: C.qkv_norm_rope_fwd(qkv, wq, wk, cos, sin, None,
                                                 Hq, Hkv, D, eps),
        "fused_bwd": lambda: C.qkv_norm_rope_bwd(dq, dk, dv, qkv, wq, wk, cos,
                                                 sin, None, eps),
        "rope_fwd": lambda: C.qkv_rope_fwd(qkv, cos, sin, None, Hq, Hkv, D),
        "rope_bwd": lambda: C.qkv_rope_bwd(dq, dk, dv, cos, sin, None),
        "unfused_fwd": unfused_fwd,   # always directly before unfused_bwd
        "unfused_bwd": unfused_bwd,
    }

    times = {k: [] for k in variants}
    for it in range(args.warmup + args.repeats):
        for name, fn in variants.items():  # alternate within the run
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            if it >= args.warmup:
                times[name].append(start.elapsed_time(end))

    tokens = B * S
    result = {"tokens": tokens, "heads": Hq, "kv_heads": Hkv, "head_dim": D,
              "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0)}
    spread = {}
    for name, ts in times.items():
        result[f"{name}_ms"] = round(statistics.median(ts), 4)
        result[f"{name}_min_ms"] = round(min(ts), 4)
        result[f"{name}_max_ms"] = round(max(ts), 4)
        spread[name] = max(ts) - min(ts)
    fwd_bytes = 2 * W * 2
    bwd_bytes = (3 * Hq + 5 * Hkv) * D * 2
    for name, nbytes in (("fused_fwd", fwd_bytes), ("fused_bwd", bwd_bytes),
                         ("rope_fwd", fwd_bytes), ("rope_bwd", fwd_bytes)):
        result[f"{name}_tb_per_s"] = round(
            nbytes * tokens / (result[f"{name}_ms"] * 1e-3) / 1e12, 3)
    result["bwd_byte_ratio"] = round(bwd_bytes / fwd_bytes, 4)
    fused = result["fused_fwd_ms"] + result["fused_bwd_ms"]
    unfused = result["unfused_fwd_ms"] + result["unfused_bwd_ms"]
    all_spread = sum(spread[k] for k in ("fused_fwd", "fused_bwd",
                                         "unfused_fwd", "unfused_bwd"))
    result["fused_fwdbwd_ms"] = round(fused, 4)
    result["unfused_fwdbwd_ms"] = round(unfused, 4)
    result["fwdbwd_spread_ms"] = round(all_spread, 4)
    result["fused_beats_unfused"] = bool(unfused - fused > all_spread)
    fwd_spread = spread["fused_fwd"] + spread["rope_fwd"]
    result["fwd_spread_ms"] = round(fwd_spread, 4)
    result["fused_fwd_slower_than_rope_fwd"] = bool(
        result["fused_fwd_ms"] - result["rope_fwd_ms"] > fwd_spread)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged["layer"] = result
    out.write_text(json.dumps(merged, indent=2) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
