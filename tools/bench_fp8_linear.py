#!/usr/bin/env python3
"""FP8 linears against bf16 on the GPU (run on a GPU box).

Per layer.  The four Llama-3-8B projections at M = 24576 rows (batch 24 x
sequence 1024), forward plus backward, `F.linear` in bf16 against
`ops.fp8_linear`; the two alternate inside one run, device events around
each call, warm-up, median of the repeats.  The quantisation kernels of one
fp8 forward+backward are then timed on their own (the same four calls the
autograd function makes) and reported as a share of the fp8 time and as
achieved GB/s against the bytes a two-pass scheme has to move:

    amax pass            2 B/element read
    cast, both outputs   2 B read + 2 B written
    cast, one output     2 B read + 1 B written

End to end (--e2e): 01-single-gpu/train_llm.py on synthetic llama-3-8b at
batch 24, sequence 1024, with and without --fp8, each in a fresh child
process, alternating, in this one run.  The figure is the trainer's own
time/total (phase timers fenced by device synchronisation) over the log
windows after the first.

Numbers are reported, not gated.  Writes profiles/fp8_linear.json.
"""
import argparse
import ast
import json
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch
import torch.nn.functional as F

# name -> (N, K) of this repo's packed Llama-3-8B projections
PROJECTIONS = {
    "qkv_proj": (6144, 4096),
    "o_proj": (4096, 4096),
    "gate_up_proj": (28672, 4096),
    "down_proj": (4096, 14336),
}


def quant_floor_bytes(M, N, K):
    """Bytes the quantisation of one fp8 forward+backward has to move:
    x and dy get amax + both outputs, w amax + row-major in forward and the
    transposed copy alone (saved scale) in backward."""
    both = 2 + 2 + 2
    return {"x": M * K * both, "w_fwd": N * K * (2 + 2 + 1),
            "dy": M * N * both, "w_bwd": N * K * (2 + 1)}


def timed(fn, warmup, repeats):
    ts = []
    for it in range(warmup + repeats):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        if it >= warmup:
            ts.append(start.elapsed_time(end))
    return ts


def bench_layer(name, M, N, K, warmup, repeats):
    from distributed_training_guide_amd.ops import fp8_linear, fp8_quantize

    dev = torch.device("cuda")
    x = torch.randn(M, K, device=dev).bfloat16().requires_grad_()
    w = (0.02 * torch.randn(N, K, device=dev)).bfloat16().requires_grad_()
    dy = torch.randn(M, N, device=dev).bfloat16()

    def run(linear):
        x.grad = w.grad = None
        linear(x, w).backward(dy)

    variants = {"bf16": lambda: run(F.linear), "fp8": lambda: run(fp8_linear)}
    times = {k: [] for k in variants}
    for it in range(warmup + repeats):
        for key, fn in variants.items():  # alternate within the run
            t = timed(fn, 0, 1)
            if it >= warmup:
                times[key] += t

    xd, wd = x.detach(), w.detach()
    sw = fp8_quantize(wd)[2]
    quant_calls = {
        "x": lambda: fp8_quantize(xd, True, True),
        "w_fwd": lambda: fp8_quantize(wd, True, False),
        "dy": lambda: fp8_quantize(dy, True, True),
        "w_bwd": lambda: fp8_quantize(wd, False, True, scale=sw),
    }
    floor = quant_floor_bytes(M, N, K)
    quant = {}
    for key, fn in quant_calls.items():
        ms = statistics.median(timed(fn, warmup, repeats))
        quant[key] = {"ms": round(ms, 4), "floor_bytes": floor[key],
                      "gb_per_s": round(floor[key] / (ms * 1e-3) / 1e9, 1)}
    quant_ms = sum(v["ms"] for v in quant.values())

    flops = 3 * 2 * M * N * K
    row = {"M": M, "N": N, "K": K}
    for key, ts in times.items():
        med = statistics.median(ts)
        row[f"{key}_ms"] = round(med, 4)
        row[f"{key}_min_ms"] = round(min(ts), 4)
        row[f"{key}_max_ms"] = round(max(ts), 4)
        row[f"{key}_tflops"] = round(flops / (med * 1e-3) / 1e12, 1)
    row["fp8_over_bf16"] = round(row["fp8_ms"] / row["bf16_ms"], 4)
    row["quant_ms"] = round(quant_ms, 4)
    row["quant_share_of_fp8"] = round(quant_ms / row["fp8_ms"], 4)
    row["quant_gb_per_s"] = round(
        sum(floor.values()) / (quant_ms * 1e-3) / 1e9, 1)
    row["quant"] = quant
    print(name, json.dumps(row), flush=True)
    return row


def run_trainer(fp8, model, steps, log_freq, batch, seq, timeout,
                extra=()):
    cmd = [sys.executable, str(REPO / "01-single-gpu" / "train_llm.py"),
           "-m", model, "-d", "synthetic", "-b", str(batch),
           "-s", str(seq), "--num-samples", str(batch * (steps + 2)),
           "--num-workers", "0", "--num-epochs", "1",
           "--max-steps", str(steps), "--log-freq", str(log_freq)]
    cmd += list(extra)
    if fp8:
        cmd.append("--fp8")
    proc = subprocess.run(cmd, capture_output=True, text=True,
                          timeout=timeout, cwd=REPO)
    if proc.returncode != 0:
        sys.exit(f"trainer failed (rc {proc.returncode}):\n"
                 + proc.stderr[-3000:])
    infos = [ast.literal_eval(ln.split("INFO:", 1)[1].strip())
             for ln in proc.stderr.splitlines() if "'global_step'" in ln]
    steady = infos[1:]  # the first window holds the warm-up
    if not steady:
        sys.exit("trainer logged fewer than two windows")
    return {"ms_per_step": round(statistics.mean(
                i["time/total"] for i in steady), 2),
            "tokens_per_s": round(statistics.mean(
                i["tokens_per_s"] for i in steady), 1),
            "windows_ms": [round(i["time/total"], 2) for i in steady],
            "loss_last_window": round(infos[-1]["running_loss"], 4),
            "peak_alloc_gb": infos[-1].get("peak_alloc_gb")}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=24576, help="M of every GEMM")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--e2e", action="store_true",
                   help="also run the end-to-end trainer comparison")
    p.add_argument("--e2e-model", default="llama-3-8b")
    p.add_argument("--e2e-batch", type=int, default=24)
    p.add_argument("--e2e-seq", type=int, default=1024)
    p.add_argument("--e2e-pairs", type=int, default=2)
    p.add_argument("--e2e-steps", type=int, default=12)
    p.add_argument("--e2e-log-freq", type=int, default=4)
    p.add_argument("--e2e-timeout", type=int, default=420,
                   help="seconds allowed to one trainer process")
    p.add_argument("--skip-layers", action="store_true")
    p.add_argument("--out", default="profiles/fp8_linear.json")
    args = p.parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench_fp8_linear needs a GPU: timings are not measured "
                 "on the CPU")
    from distributed_training_guide_amd._ext import ext

    ext()  # fail loudly without the HIP extension
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0),
              "torch": torch.__version__, "rows": args.rows,
              "warmup": args.warmup, "repeats": args.repeats}
    if not args.skip_layers:
        layers = {name: bench_layer(name, args.rows, N, K, args.warmup,
                                    args.repeats)
                  for name, (N, K) in PROJECTIONS.items()}
        result["layers"] = layers
        for key in ("bf16_ms", "fp8_ms", "quant_ms"):
            result[f"sum_{key}"] = round(
                sum(r[key] for r in layers.values()), 4)
        result["sum_fp8_over_bf16"] = round(
            result["sum_fp8_ms"] / result["sum_bf16_ms"], 4)
        torch.cuda.empty_cache()
    if args.e2e:
        runs = []
        for pair in range(args.e2e_pairs):
            for fp8 in (False, True):  # alternate
                r = run_trainer(fp8, args.e2e_model, args.e2e_steps,
                                args.e2e_log_freq, args.e2e_batch,
                                args.e2e_seq, args.e2e_timeout)
                r["fp8"] = fp8
                runs.append(r)
                print("e2e", json.dumps(r), flush=True)
        mean = {k: statistics.mean(r["ms_per_step"] for r in runs
                                   if r["fp8"] is k) for k in (False, True)}
        result["e2e"] = {
            "model": args.e2e_model, "batch": args.e2e_batch,
            "seq": args.e2e_seq, "runs": runs,
            "bf16_ms_per_step": round(mean[False], 2),
            "fp8_ms_per_step": round(mean[True], 2),
            "fp8_over_bf16": round(mean[True] / mean[False], 4)}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=2) + "\n")
    print(json.dumps({k: v for k, v in result.items() if k != "layers"}))


if __name__ == "__main__":
    main()
