#!/usr/bin/env python3
"""Micro-benchmark for fused gradient clipping (run on a GPU box).

Allocates a synthetic Llama-3-8B parameter set (bf16 params, bf16 grads,
fp32 moments, ~96 GB) and times one optimizer update three ways, alternating
them within one run (device events, warm-up, median of repeats):

  (a) unclipped  FusedAdamW.step
  (b) fused      FusedAdamW(max_grad_norm).step: grad_norm.hip read pass +
                 the clipped AdamW kernel, grads never rewritten
  (c) torch      torch.nn.utils.clip_grad_norm_(foreach=True), then (a)

Pass condition: (b) < (c).  Writes the medians and (b)-(a) as JSON.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


def llama_shapes(layers, hidden=4096, inter=14336, vocab=128256, hq=32,
                 hkv=8, d=128):
    """This repo's Llama-3-8B tensors: packed qkv and gate|up."""
    shapes = [(vocab, hidden)]
    for _ in range(layers):
        shapes += [(hidden,), ((hq + 2 * hkv) * d, hidden),
                   (hidden, hq * d), (hidden,), (2 * inter, hidden),
                   (hidden, inter)]
    shapes += [(hidden,), (vocab, hidden)]
    return shapes


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=32,
                   help="decoder layers (32 = Llama-3-8B; fewer to rehearse)")
    p.add_argument("--max-norm", type=float, default=1.0)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=15)
    p.add_argument("--out", default="profiles/grad_clip.json")
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_grad_clip needs a GPU: timings are not measured "
                 "on the CPU")
    from distributed_training_guide_amd._ext import ext
    from distributed_training_guide_amd.ops import FusedAdamW

    ext()  # fail loudly without the HIP extension
    torch.manual_seed(0)
    dev = torch.device("cuda")
    params = [torch.empty(s, device=dev, dtype=torch.bfloat16)
              .normal_(0, 0.02).requires_grad_(True)
              for s in llama_shapes(args.layers)]
    for q in params:
        q.grad = torch.empty_like(q).normal_(0, 1e-3)
    n_params = sum(q.numel() for q in params)
    opt = FusedAdamW(params, lr=3e-5)
    group = opt.param_groups[0]

    def unclipped():
        group["max_grad_norm"] = 0.0
        opt.step()

    def fused():
        group["max_grad_norm"] = args.max_norm
        opt.step()

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(params, args.max_norm, foreach=True)
        unclipped()

    variants = {"unclipped_ms": unclipped, "fused_clipped_ms": fused,
                "torch_clip_then_step_ms": torch_clip}
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

    result = {"n_params": n_params, "layers": args.layers,
              "max_norm": args.max_norm, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        result[name] = round(statistics.median(ts), 4)
        result[name.replace("_ms", "_min_ms")] = round(min(ts), 4)
        result[name.replace("_ms", "_max_ms")] = round(max(ts), 4)
    result["fused_minus_unclipped_ms"] = round(
        result["fused_clipped_ms"] - result["unclipped_ms"], 4)
    # bytes the algorithm needs: update = p r/w (2+2) + g (2) + m, v r/w
    # (16) = 22 B/param; the norm pass reads g again (2 B/param)
    result["unclipped_tb_per_s"] = round(
        22 * n_params / (result["unclipped_ms"] * 1e-3) / 1e12, 3)
    result["fused_clipped_tb_per_s"] = round(
        24 * n_params / (result["fused_clipped_ms"] * 1e-3) / 1e12, 3)
    result["grad_norm"] = opt.last_grad_norm.item()
    result["pass"] = (result["fused_clipped_ms"]
                      < result["torch_clip_then_step_ms"])
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps(result))
    if not result["pass"]:
        sys.exit("FAIL: fused clipped step is not faster than "
                 "torch clip_grad_norm_ + step")


if __name__ == "__main__":
    main()
