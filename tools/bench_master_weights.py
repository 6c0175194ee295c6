#!/usr/bin/env python3
"""Micro-benchmark for the master-weight AdamW update (run on a GPU box).

Allocates the synthetic Llama-3-8B parameter set of tools/bench_grad_clip.py
(bf16 params and grads, fp32 moments, plus the int16 companions: ~112 GB)
and times one optimizer update four ways, alternating them within one run
(device events, warm-up, median of repeats):

  plain            FusedAdamW.step                           22 B/element
  plain_clipped    ... with max_grad_norm (grad_norm.hip pass + CLIP kernel)
  master           FusedAdamW(master_weights=True).step      26 B/element
  master_clipped   ... with max_grad_norm

The two optimizers share parameters, gradients and moments, so the set is
allocated once.  --baseline-ext PATH loads the _C.so of another build (the
parent commit's, say) and times its adamw_step on the same descriptor table,
alternating with this tree's, both through the raw binding: the default
path's code is meant to be unchanged, and this is where that shows.

Writes the medians, the achieved bytes/s and the master / plain ratio (the
byte ratio is 26/22 = 1.18) into the JSON file, keeping any other keys the
file already holds.
"""
import argparse
import importlib.util
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch

from bench_grad_clip import llama_shapes


def load_ext(path):
    spec = importlib.util.spec_from_file_location("_C", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=32,
                   help="decoder layers (32 = Llama-3-8B; fewer to rehearse)")
    p.add_argument("--max-norm", type=float, default=1.0)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=15)
    p.add_argument("--baseline-ext", default=None,
                   help="_C.so of another build, timed against this one's")
    p.add_argument("--out", default="profiles/master_weights.json")
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_master_weights needs a GPU: timings are not "
                 "measured on the CPU")
    from distributed_training_guide_amd._ext import ext
    from distributed_training_guide_amd.ops import FusedAdamW

    cur = ext()  # fail loudly without the HIP extension
    torch.manual_seed(0)
    dev = torch.device("cuda")
    params = [torch.empty(s, device=dev, dtype=torch.bfloat16)
              .normal_(0, 0.02).requires_grad_(True)
              for s in llama_shapes(args.layers)]
    for q in params:
        q.grad = torch.empty_like(q).normal_(0, 1e-3)
    n_params = sum(q.numel() for q in params)
    plain = FusedAdamW(params, lr=3e-5)
    master = FusedAdamW(params, lr=3e-5, master_weights=True)
    plain.step()
    for q in params:  # one set of moments for both
        for key in ("exp_avg", "exp_avg_sq"):
            master.state[q][key] = plain.state[q][key]

    def stepper(opt, max_norm):
        def run():
            opt.param_groups[0]["max_grad_norm"] = max_norm
            opt.step()
        return run

    variants = {"plain_ms": stepper(plain, 0.0),
                "plain_clipped_ms": stepper(plain, args.max_norm),
                "master_ms": stepper(master, 0.0),
                "master_clipped_ms": stepper(master, args.max_norm)}
    if args.baseline_ext:
        base = load_ext(args.baseline_ext)
        _, desc, nchunks, _ = plain._desc_cache[0]
        g = plain.param_groups[0]

        def raw(mod):
            def run():
                mod.adamw_step(desc, nchunks, g["lr"], *g["betas"], g["eps"],
                               g["weight_decay"], max(g["step"], 1))
            return run
        variants["raw_plain_ms"] = raw(cur)
        variants["baseline_raw_plain_ms"] = raw(base)

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
    # bytes the algorithm needs per element: p r/w (2+2), g (2), m and v
    # r/w (16) = 22; the companion r/w adds 4; the norm pass reads g again
    for name, nbytes in (("plain", 22), ("plain_clipped", 24),
                         ("master", 26), ("master_clipped", 28)):
        result[f"{name}_tb_per_s"] = round(
            nbytes * n_params / (result[f"{name}_ms"] * 1e-3) / 1e12, 3)
    result["master_over_plain"] = round(
        result["master_ms"] / result["plain_ms"], 4)
    result["master_clipped_over_plain_clipped"] = round(
        result["master_clipped_ms"] / result["plain_clipped_ms"], 4)
    result["byte_ratio"] = round(26 / 22, 4)
    if args.baseline_ext:
        result["raw_plain_over_baseline"] = round(
            result["raw_plain_ms"] / result["baseline_raw_plain_ms"], 4)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged["update"] = result
    out.write_text(json.dumps(merged, indent=2) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
