#!/usr/bin/env python3
"""Micro-benchmark for the embedding backward variants (run on a GPU box).

At one table's shape (default: the padded Llama-3 vocabulary, V 128256,
H 4096, 24576 tokens) and for three id distributions (uniform, Zipf with
s = 1 over a shuffled vocabulary, all ids equal) it times, alternating the
variants within one process (device events, warm-up, median / min / max of
the repeats):

  atomic   embedding.hip: cleared f32 [V, H] workspace, f32 atomics, convert
  sorted   embedding_bwd_sorted.hip: stable sort of the positions by id, one
           wave per table row, no atomics, a fixed summation order
  sorted_det  the same call with torch.use_deterministic_algorithms(True),
           as the determinism recipe runs it: torch then fills every
           torch.empty buffer, the returned gradient included, before the
           kernels overwrite it
  torch    autograd's backward of F.embedding under that flag: what the
           determinism recipe ran before `sorted` existed

The byte floor of the operation is one write of the bf16 gradient and one
read of dy, 2 * V * H + 2 * N * H; the rate reported is that floor over the
median time.  Peak-allocation deltas of one call are recorded for atomic and
sorted (torch.cuda.max_memory_allocated around the call; both include the
returned [V, H] bf16 gradient).

The acceptance condition is recorded in the JSON, not a preset number:
`sorted_slower_than_torch` (and `sorted_det_slower_than_torch`) is true for
a distribution when that variant trails torch's deterministic backward by
more than the two variants' joint min-max spread.  sorted against atomic is
reported only."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch
import torch.nn.functional as F


def make_ids(kind, N, V, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    if kind == "uniform":
        ids = torch.randint(0, V, (N,), generator=g)
    elif kind == "zipf":
        rank = torch.multinomial(1.0 / torch.arange(1, V + 1).double(), N,
                                 replacement=True, generator=g)
        ids = torch.randperm(V, generator=g)[rank]
    else:
        ids = torch.full((N,), V // 2, dtype=torch.int64)
    return ids.to(dev)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--vocab", type=int, default=128256)
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--tokens", type=int, default=24576)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--out", default="profiles/embedding_sorted.json")
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_embedding needs a GPU: timings are not measured on "
                 "the CPU")
    from distributed_training_guide_amd._ext import ext

    C = ext()  # fail loudly without the HIP extension
    dev = torch.device("cuda")
    V, H, N = args.vocab, args.hidden, args.tokens
    torch.manual_seed(0)
    dy = torch.randn(N, H, device=dev, dtype=torch.bfloat16)
    table = torch.zeros(V, H, device=dev, dtype=torch.bfloat16,
                        requires_grad=True)
    floor = 2 * V * H + 2 * N * H
    result = {"vocab": V, "hidden": H, "tokens": N, "repeats": args.repeats,
              "floor_bytes": floor, "device": torch.cuda.get_device_name(0)}

    for kind in ("uniform", "zipf", "equal"):
        ids = make_ids(kind, N, V, dev)
        out = F.embedding(ids, table)

        def under_flag(fn):
            def run():
                torch.use_deterministic_algorithms(True)
                try:
                    return fn()
                finally:
                    torch.use_deterministic_algorithms(False)
            return run

        variants = {
            "atomic": lambda: C.embedding_bwd(dy, ids, V),
            "sorted": lambda: C.embedding_bwd_sorted(dy, ids, V),
            "sorted_det": under_flag(
                lambda: C.embedding_bwd_sorted(dy, ids, V)),
            "torch": under_flag(lambda: torch.autograd.grad(
                out, table, dy, retain_graph=True)),
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
        r = {"distinct_ids": int(ids.unique().numel()),
             "max_hits_per_row": int(torch.bincount(ids).max().item())}
        for name, ts in times.items():
            r[f"{name}_ms"] = round(statistics.median(ts), 4)
            r[f"{name}_min_ms"] = round(min(ts), 4)
            r[f"{name}_max_ms"] = round(max(ts), 4)
            r[f"{name}_tb_per_s"] = round(
                floor / (statistics.median(ts) * 1e-3) / 1e12, 3)
        for name in ("sorted", "sorted_det"):
            spread = sum(max(times[k]) - min(times[k]) for k in (name, "torch"))
            r[f"{name}_torch_spread_ms"] = round(spread, 4)
            r[f"{name}_slower_than_torch"] = bool(
                r[f"{name}_ms"] - r["torch_ms"] > spread)
        for name in ("atomic", "sorted"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            g = variants[name]()
            torch.cuda.synchronize()
            r[f"{name}_peak_alloc_delta_mb"] = round(
                (torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            del g
        result[kind] = r
        del out

    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    merged = json.loads(path.read_text()) if path.exists() else {}
    merged["per_call"] = result
    path.write_text(json.dumps(merged, indent=2) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
