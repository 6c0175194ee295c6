#!/usr/bin/env python3
"""Micro-benchmark for the mixture-of-experts kernels (run on a GPU box).

At one MoE layer's shape (default: Qwen3-30B-A3B at 24576 tokens, H 2048,
I 768, E 128, k 8) it times, alternating the variants within one process
(device events, warm-up, median / min / max of the repeats), each fused op
against the torch-op chain it replaces:

  router_fwd / router_bwd     moe_router.hip | softmax / sort / gather
  index                       moe_dispatch.hip's three launches | stable sort
                              + bincount + cumsum
                              (these take tens of microseconds on inputs
                              that stay in cache: 20 launches per event
                              pair, reported per launch)
  scatter_fwd / scatter_bwd   row scatter and its backward (the k-way sum)
                              | index_select and its bf16 index_add_
  combine_fwd / combine_bwd   weighted combine and its one-pass backward
                              | gather, multiply, f32 index_add_ and
                              autograd's backward of that
  path_fwdbwd                 router to combine around the expert GEMMs,
                              forward and backward | the same as torch ops
  gemm_fwdbwd                 the two expert GEMMs and silu_mul alone,
                              forward and backward (part of both paths)

Byte floors (bf16 rows of H, N = T*k slots): scatter forward reads T and
writes N rows; its backward reads N and writes T; combine forward reads N
and writes T; combine backward reads T + N and writes N.  The fused ops'
rates against those floors are reported in TB/s.

--aux times the router with its auxiliary losses instead (moe_router_aux.hip,
default --out profiles/moe_aux.json), alternating in one run: the plain
router fwd / bwd of this build, the aux fwd (with its finishing launch) / bwd,
and the torch-op chain for the same two losses from the logits and the
selection (logsumexp, exp, bincount, two means) with autograd's backward.

--expert-gemm times the expert GEMMs instead (default --out
profiles/moe_gemm.json), alternating in one run: forward, dA and dW of the
gate_up and the down GEMM as torch's grouped GEMM and as moe_gemm.hip, with
the achieved TFLOP/s from the shapes (2 N M K per product), and the whole
layer forward + backward with either.

--gather times expert_gemm="hip-gather" against "hip" instead (default --out
profiles/moe_gemm_gather.json), alternating in one run: the gate_up forward
of moe_gemm_gather.hip against scatter + forward, the gate_up dW both ways,
the row index build, the whole layer forward + backward, and the memory a
layer holds after its forward and at its peak.

--fused times expert_gemm="hip-fused" against "hip-gather" instead (default
--out profiles/moe_gemm_swiglu.json), alternating in one run: the gate_up
forward with the SwiGLU epilogue against gather forward + silu_mul, the down
dA with the SwiGLU-backward epilogue + the unweighted scatter against dA +
silu_mul backward + the combine's backward, the whole layer forward +
backward, and the memory a layer holds after its forward and at its peak.

--e2e-layers L additionally times training steps of a cut-down model of the
same layer shape with L layers (the 30B model's 366 GB of parameter and
optimizer state do not fit one GPU).  Results go to --out; no threshold is
asserted."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch


# launches per event pair for the ops that take tens of microseconds (router,
# index build): one launch between two events would time the events
SMALL_OP_LAUNCHES = 20


def timed(variants, warmup, repeats):
    """variants: name -> fn or (fn, launches per event pair); times are per
    launch."""
    times = {k: [] for k in variants}
    for it in range(warmup + repeats):
        for name, v in variants.items():  # alternate within the run
            fn, inner = v if isinstance(v, tuple) else (v, 1)
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(inner):
                fn()
            end.record()
            end.synchronize()
            if it >= warmup:
                times[name].append(start.elapsed_time(end) / inner)
    out = {}
    for name, ts in times.items():
        out[f"{name}_ms"] = round(statistics.median(ts), 4)
        out[f"{name}_min_ms"] = round(min(ts), 4)
        out[f"{name}_max_ms"] = round(max(ts), 4)
    return out


def e2e(args, dev):
    from distributed_training_guide_amd.models import build_model
    from distributed_training_guide_amd.models.llama import LlamaConfig
    from distributed_training_guide_amd.ops import FusedAdamW

    cfg = LlamaConfig(
        vocab_size=151936, hidden_size=args.hidden, intermediate_size=args.inter,
        num_hidden_layers=args.e2e_layers, num_attention_heads=32,
        num_key_value_heads=4, max_position_embeddings=40960, rope_theta=1e6,
        rms_norm_eps=1e-6, qk_norm=True, head_dim_override=128,
        num_experts=args.experts, num_experts_per_tok=args.top_k,
        moe_intermediate_size=args.inter)
    model = build_model(cfg, device=dev, dtype=torch.bfloat16)
    opt = FusedAdamW(model.parameters(), lr=1e-4)
    seq = 4096
    ids = torch.randint(0, cfg.vocab_size, (args.tokens // seq, seq),
                        device=dev)
    steps = []
    for it in range(2 + args.e2e_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = model(input_ids=ids, labels=ids).loss
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        if it >= 2:
            steps.append((time.perf_counter() - t0) * 1e3)
    return {"layers": args.e2e_layers, "tokens": ids.numel(),
            "parameters": cfg.num_parameters(),
            "step_ms": round(statistics.median(steps), 2),
            "step_min_ms": round(min(steps), 2),
            "step_max_ms": round(max(steps), 2),
            "tokens_per_s": round(ids.numel() / statistics.median(steps) * 1e3),
            "final_loss": round(loss.item(), 4),
            "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1)}


def expert_gemm_mode(args, C, moe, silu_mul, x, router_w, gate_up, down, xp,
                     offs, dy, fwd, bwd):
    """The six products of the two expert GEMMs (forward, dA, dW of gate_up
    [E, 2I, H] and down [E, H, I]) as torch's grouped GEMM and as
    moe_gemm.hip, alternating in one run, and the whole layer both ways.
    torch's dA / dW are autograd's backward of F.grouped_mm with only that
    input requiring a gradient; the hip products are the kernels themselves."""
    k = args.top_k
    N = xp.shape[0]
    h = silu_mul(moe.expert_mm(xp, gate_up, offs))
    variants, flops, check = {}, {}, {}
    for name, a, w in (("gate_up", xp, gate_up), ("down", h, down)):
        M, K = w.shape[1], w.shape[2]
        g = torch.randn(N, M, device=a.device, dtype=a.dtype)
        flops[name] = 2.0 * N * M * K
        # the timed products agree at the timed shape: largest difference
        # between the two implementations over the largest value
        al, wl = a.detach().requires_grad_(), w.detach().requires_grad_()
        ref = moe.expert_mm(al, wl, offs)
        ref.backward(g)
        for prod, want, got in (
                ("fwd", ref.detach(), C.moe_gemm_rows(a, w, offs, False)),
                ("da", al.grad, C.moe_gemm_rows(g, w, offs, True)),
                ("dw", wl.grad, C.moe_gemm_dw(g, a, offs))):
            check[f"{name}_{prod}_max_diff_over_max"] = round(
                ((got.float() - want.float()).abs().max()
                 / want.float().abs().max()).item(), 5)
        del al, wl, ref
        variants.update({
            f"torch_{name}_fwd": lambda a=a, w=w: moe.expert_mm(a, w, offs),
            f"hip_{name}_fwd":
                lambda a=a, w=w: C.moe_gemm_rows(a, w, offs, False),
            f"torch_{name}_da_fwd": fwd(
                f"a{name}", lambda a_, w=w: moe.expert_mm(a_, w, offs), a),
            f"torch_{name}_da": bwd(f"a{name}", g),
            f"hip_{name}_da":
                lambda g=g, w=w: C.moe_gemm_rows(g, w, offs, True),
            f"torch_{name}_dw_fwd": fwd(
                f"w{name}", lambda w_, a=a: moe.expert_mm(a, w_, offs), w),
            f"torch_{name}_dw": bwd(f"w{name}", g),
            f"hip_{name}_dw": lambda g=g, a=a: C.moe_gemm_dw(g, a, offs),
        })
    for impl in ("torch", "hip"):
        variants[f"{impl}_layer_fwd"] = fwd(
            impl, lambda *a, impl=impl: moe.moe_mlp(*a, k, True,
                                                    expert_gemm=impl),
            x, router_w, gate_up, down)
        variants[f"{impl}_layer_bwd"] = bwd(impl, dy)
    res = timed(variants, args.warmup, args.repeats)
    res.update(check)
    for name, fl in flops.items():
        for pre in ("torch", "hip"):
            for prod in ("fwd", "da", "dw"):
                ms = res.get(f"{pre}_{name}_{prod}_ms")
                if ms:
                    res[f"{pre}_{name}_{prod}_tflops"] = round(
                        fl / (ms * 1e-3) / 1e12, 1)
    for impl in ("torch", "hip"):
        res[f"{impl}_layer_fwdbwd_ms"] = round(
            res[f"{impl}_layer_fwd_ms"] + res[f"{impl}_layer_bwd_ms"], 4)
        res[f"{impl}_six_products_ms"] = round(sum(
            res[f"{impl}_{n}_{p}_ms"] for n in flops
            for p in ("fwd", "da", "dw")), 4)
    rows = torch.diff(offs, prepend=offs.new_zeros(1))
    res["rows_per_expert_min_mean_max"] = [
        rows.min().item(), round(N / offs.numel(), 1), rows.max().item()]
    return res


def gather_mode(args, C, moe, x, router_w, gate_up, down, dest, offs, dy, fwd,
                bwd):
    """expert_gemm="hip-gather" against "hip", alternating in one run: the
    gate_up forward reading x through row_src against scatter + forward on
    the copy, the gate_up dW both ways, the row index build, the whole layer
    forward + backward, and the peak allocation of one layer step above what
    is allocated before it."""
    k = args.top_k
    N = dest.numel()
    row_src = C.moe_row_src(dest, k)
    xp = C.moe_scatter(x, dest)
    g = torch.randn(N, gate_up.shape[1], device=x.device, dtype=x.dtype)
    same = {
        "fwd_equal": torch.equal(
            C.moe_gemm_rows_gather(x, row_src, gate_up, offs),
            C.moe_gemm_rows(xp, gate_up, offs, False)),
        "dw_equal": torch.equal(C.moe_gemm_dw_gather(g, x, row_src, offs),
                                C.moe_gemm_dw(g, xp, offs)),
    }
    variants = {
        "row_src": (lambda: C.moe_row_src(dest, k), SMALL_OP_LAUNCHES),
        "hip_scatter_fwd": lambda: C.moe_gemm_rows(
            C.moe_scatter(x, dest), gate_up, offs, False),
        "gather_fwd": lambda: C.moe_gemm_rows_gather(x, row_src, gate_up,
                                                     offs),
        "hip_dw": lambda: C.moe_gemm_dw(g, xp, offs),
        "gather_dw": lambda: C.moe_gemm_dw_gather(g, x, row_src, offs),
    }
    impls = ("hip", "hip-gather")
    variants.update(layer_variants(args, moe, impls, x, router_w, gate_up,
                                   down, dy, fwd, bwd))
    res = timed(variants, args.warmup, args.repeats)
    res.update(same)
    del xp, g
    layer_memory(res, impls, variants)
    return res


def layer_variants(args, moe, impls, x, router_w, gate_up, down, dy, fwd, bwd):
    return {f"{impl}_layer_{d}": v for impl in impls for d, v in (
        ("fwd", fwd(impl, lambda *a, impl=impl: moe.moe_mlp(
            *a, args.top_k, True, expert_gemm=impl), x, router_w, gate_up,
            down)),
        ("bwd", bwd(impl, dy)))}


def layer_memory(res, impls, variants):
    """fwd+bwd sums, and a layer step's held and peak allocation above what
    is allocated before it"""
    for impl in impls:
        res[f"{impl}_layer_fwdbwd_ms"] = round(
            res[f"{impl}_layer_fwd_ms"] + res[f"{impl}_layer_bwd_ms"], 4)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        variants[f"{impl}_layer_fwd"]()
        held = torch.cuda.memory_allocated() - base
        variants[f"{impl}_layer_bwd"]()
        torch.cuda.synchronize()
        res[f"{impl}_layer_held_after_fwd_mb"] = round(held / 1e6, 1)
        res[f"{impl}_layer_peak_mb"] = round(
            (torch.cuda.max_memory_allocated() - base) / 1e6, 1)


def fused_mode(args, C, moe, x, router_w, gate_up, down, dest, offs, w, dy,
               fwd, bwd):
    """expert_gemm="hip-fused" against "hip-gather", alternating in one run:
    the two epilogue-fused kernels of moe_gemm_swiglu.hip against the kernels
    they replace, the whole layer, and its memory."""
    k = args.top_k
    N = dest.numel()
    row_src, w_row = C.moe_row_src(dest, k), C.moe_row_w(dest, w)
    gu, hw = C.moe_gemm_gu_swiglu(x, row_src, w_row, gate_up, offs)
    yp = C.moe_gemm_rows(hw, down, offs, False)
    dyp = torch.randn(N, x.shape[1], device=x.device, dtype=x.dtype)
    res = {"gu_equal": torch.equal(
        gu, C.moe_gemm_rows_gather(x, row_src, gate_up, offs))}

    def gather_bwd():
        dyp_, _ = C.moe_combine_bwd(dy, dest, w, yp)
        return C.silu_mul_bwd(C.moe_gemm_rows(dyp_, down, offs, True), gu)

    variants = {
        "row_w": (lambda: C.moe_row_w(dest, w), SMALL_OP_LAUNCHES),
        "gather_fwd_silu": lambda: C.silu_mul_fwd(
            C.moe_gemm_rows_gather(x, row_src, gate_up, offs)),
        "fused_fwd": lambda: C.moe_gemm_gu_swiglu(x, row_src, w_row, gate_up,
                                                  offs),
        "gather_combine_bwd_da_silu_bwd": gather_bwd,
        "fused_scatter_da": lambda: C.moe_gemm_da_swiglu(
            C.moe_scatter(dy, dest), down, gu, w_row, offs, dest),
        "hip_da": lambda: C.moe_gemm_rows(dyp, down, offs, True),
        "fused_da": lambda: C.moe_gemm_da_swiglu(dyp, down, gu, w_row, offs,
                                                 dest),
    }
    impls = ("hip-gather", "hip-fused")
    variants.update(layer_variants(args, moe, impls, x, router_w, gate_up,
                                   down, dy, fwd, bwd))
    res.update(timed(variants, args.warmup, args.repeats))
    del gu, hw, yp, dyp
    layer_memory(res, impls, variants)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tokens", type=int, default=24576)
    p.add_argument("--hidden", type=int, default=2048)
    p.add_argument("--inter", type=int, default=768)
    p.add_argument("--experts", type=int, default=128)
    p.add_argument("--top-k", type=int, default=8)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--e2e-layers", type=int, default=0)
    p.add_argument("--e2e-steps", type=int, default=5)
    p.add_argument("--aux", action="store_true",
                   help="time the router's auxiliary-loss variants only")
    p.add_argument("--expert-gemm", action="store_true",
                   help="time the expert GEMMs only: torch's grouped GEMM "
                        "against _hip/moe_gemm.hip")
    p.add_argument("--gather", action="store_true",
                   help="time expert_gemm='hip-gather' "
                        "(_hip/moe_gemm_gather.hip) against 'hip'")
    p.add_argument("--fused", action="store_true",
                   help="time expert_gemm='hip-fused' "
                        "(_hip/moe_gemm_swiglu.hip) against 'hip-gather'")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.out is None:
        args.out = "profiles/moe_aux.json" if args.aux else \
            "profiles/moe_gemm.json" if args.expert_gemm else \
            "profiles/moe_gemm_gather.json" if args.gather else \
            "profiles/moe_gemm_swiglu.json" if args.fused else \
            "profiles/moe.json"

    if not torch.cuda.is_available():
        sys.exit("bench_moe needs a GPU: timings are not measured on the CPU")
    from distributed_training_guide_amd._ext import ext
    from distributed_training_guide_amd.ops import moe, silu_mul

    C = ext()  # fail loudly without the HIP extension
    torch.manual_seed(0)
    dev = torch.device("cuda")
    T, H, I, E, k = (args.tokens, args.hidden, args.inter, args.experts,
                     args.top_k)
    N = T * k
    bf = dict(device=dev, dtype=torch.bfloat16)
    x = torch.randn(T, H, **bf)
    router_w = torch.randn(E, H, **bf) * 0.05
    gate_up = torch.randn(E, 2 * I, H, **bf) * 0.02
    down = torch.randn(E, H, I, **bf) * 0.02
    logits = torch.nn.functional.linear(x, router_w)
    dy = torch.randn(T, H, **bf)
    idx, w = C.moe_router_fwd(logits, k, True)
    idx64 = idx.reshape(-1).long()  # what torch.bincount takes
    dest, offs = C.moe_dispatch_index(idx, E)
    dw = torch.randn(T, k, device=dev)
    yp = torch.randn(N, H, **bf)
    dxp = torch.randn(N, H, **bf)

    graph = {}

    def fwd(key, fn, *leaves):
        """run fn on fresh leaves and keep the output for the paired bwd"""
        def run():
            ins = [t.detach().requires_grad_() for t in leaves]
            graph.setdefault(key, []).append(fn(*ins))
        return run

    def bwd(key, grad):
        return lambda: graph[key].pop().backward(grad)

    def t_router(lg):
        return moe.moe_router_eager(lg, k, True)[1]

    def t_aux(lg):
        """the two losses as torch ops; the selection is given"""
        xf = lg.float()
        lse = torch.logsumexp(xf, dim=-1)
        frac = torch.bincount(idx64, minlength=E).float() / T
        aux = E * (frac * torch.exp(xf - lse.unsqueeze(1)).mean(0)).sum()
        return aux + lse.square().mean()

    def gemms(xp_, gu_, dn_):
        return moe.expert_mm(silu_mul(moe.expert_mm(xp_, gu_, offs)), dn_,
                             offs)

    xp = C.moe_scatter(x, dest)
    dyp = torch.randn(N, H, **bf)
    dlogits = torch.randn(T, E, **bf)
    n = SMALL_OP_LAUNCHES
    variants = {
        "router_fwd": (lambda: C.moe_router_fwd(logits, k, True), n),
        "router_bwd": (lambda: C.moe_router_bwd(logits, idx, dw, True), n),
        "torch_router_fwd": (fwd("r", t_router, logits), n),
        "torch_router_bwd": (bwd("r", dw), n),
        "index": (lambda: C.moe_dispatch_index(idx, E), n),
        "torch_index": (lambda: moe.moe_dispatch_index_eager(idx, E), n),
        "router_gemm_fwd": fwd("rg", torch.nn.functional.linear, x, router_w),
        "router_gemm_bwd": bwd("rg", dlogits),
        "scatter_fwd": lambda: C.moe_scatter(x, dest),
        "scatter_bwd": lambda: C.moe_combine(dxp, dest, None, k),
        "torch_scatter_fwd": fwd(
            "s", lambda a: moe.moe_scatter_eager(a, dest, k), x),
        "torch_scatter_bwd": bwd("s", dxp),
        "combine_fwd": lambda: C.moe_combine(yp, dest, w, k),
        "combine_bwd": lambda: C.moe_combine_bwd(dy, dest, w, yp),
        "torch_combine_fwd": fwd(
            "c", lambda a, b: moe.moe_combine_eager(a, dest, b), yp, w),
        "torch_combine_bwd": bwd("c", dy),
        "path_fwd": fwd("p", lambda *a: moe.moe_mlp(*a, k, True), x,
                        router_w, gate_up, down),
        "path_bwd": bwd("p", dy),
        "torch_path_fwd": fwd("tp", lambda *a: moe.moe_mlp_eager(*a, k, True),
                              x, router_w, gate_up, down),
        "torch_path_bwd": bwd("tp", dy),
        "gemm_fwd": fwd("g", gemms, xp, gate_up, down),
        "gemm_bwd": bwd("g", dyp),
    }
    result = {"tokens": T, "hidden": H, "moe_intermediate": I, "experts": E,
              "top_k": k, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0)}
    if args.aux:
        counts = C.moe_router_aux_fwd(logits, k, True)[2]
        one = torch.ones((), device=dev)
        variants = {
            "router_fwd": variants["router_fwd"],
            "router_bwd": variants["router_bwd"],
            "aux_router_fwd": (lambda: C.moe_router_aux_fwd(logits, k, True),
                               n),
            "aux_router_bwd": (lambda: C.moe_router_aux_bwd(
                logits, idx, dw, counts, one, one, True), n),
            "torch_aux_fwd": (fwd("a", t_aux, logits), n),
            "torch_aux_bwd": (bwd("a", one), n),
        }
        result.update(timed(variants, args.warmup, args.repeats))
        for pre in ("router", "aux_router", "torch_aux"):
            result[f"{pre}_fwdbwd_ms"] = round(
                result[f"{pre}_fwd_ms"] + result[f"{pre}_bwd_ms"], 4)
        result["aux_over_plain"] = round(
            result["aux_router_fwdbwd_ms"] / result["router_fwdbwd_ms"], 3)
        print(json.dumps(result))
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps({"router_aux": result}, indent=2) + "\n")
        return
    if args.expert_gemm:
        del yp, dxp, dyp
        result.update(expert_gemm_mode(args, C, moe, silu_mul, x, router_w,
                                       gate_up, down, xp, offs, dy, fwd, bwd))
        print(json.dumps(result))
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps({"expert_gemm": result}, indent=2) + "\n")
        return
    if args.gather:
        del yp, dxp, dyp, xp
        result.update(gather_mode(args, C, moe, x, router_w, gate_up, down,
                                  dest, offs, dy, fwd, bwd))
        print(json.dumps(result))
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps({"gather": result}, indent=2) + "\n")
        return
    if args.fused:
        del yp, dxp, dyp, xp
        result.update(fused_mode(args, C, moe, x, router_w, gate_up, down,
                                 dest, offs, w, dy, fwd, bwd))
        print(json.dumps(result))
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps({"fused": result}, indent=2) + "\n")
        return
    result.update(timed(variants, args.warmup, args.repeats))
    result["expert_gemm_path"] = moe.last_expert_mm_path
    row = H * 2
    floors = {"scatter_fwd": (T + N) * row, "scatter_bwd": (N + T) * row,
              "combine_fwd": (N + T) * row, "combine_bwd": (T + 2 * N) * row}
    for name, nbytes in floors.items():
        result[f"{name}_floor_mb"] = round(nbytes / 1e6, 1)
        for pre in ("", "torch_"):
            result[f"{pre}{name}_tb_per_s"] = round(
                nbytes / (result[f"{pre}{name}_ms"] * 1e-3) / 1e12, 3)
    for pre in ("", "torch_"):
        total = result[f"{pre}path_fwd_ms"] + result[f"{pre}path_bwd_ms"]
        result[f"{pre}path_fwdbwd_ms"] = round(total, 4)
    gemm = result["gemm_fwd_ms"] + result["gemm_bwd_ms"]
    result["gemm_fwdbwd_ms"] = round(gemm, 4)
    # The path figures contain the router GEMM (forward and backward) as
    # well; "around_gemms" subtracts the expert GEMMs only, "around_all_gemms"
    # the router GEMM too.  Both are differences of medians of ~18 ms: their
    # spread is the summed max - min of the four timings they come from.
    rg = result["router_gemm_fwd_ms"] + result["router_gemm_bwd_ms"]
    result["router_gemm_fwdbwd_ms"] = round(rg, 4)
    for pre in ("", "torch_"):
        around = result[f"{pre}path_fwdbwd_ms"] - gemm
        result[f"{pre}path_around_gemms_ms"] = round(around, 4)
        result[f"{pre}path_around_all_gemms_ms"] = round(around - rg, 4)
        result[f"{pre}path_around_gemms_spread_ms"] = round(sum(
            result[f"{v}_max_ms"] - result[f"{v}_min_ms"]
            for v in (f"{pre}path_fwd", f"{pre}path_bwd", "gemm_fwd",
                      "gemm_bwd")), 4)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    merged = json.loads(out.read_text()) if out.exists() else {}
    merged["layer"] = result
    print(json.dumps(result))
    if args.e2e_layers > 0:
        del x, yp, dxp, dyp, xp, gate_up, down, variants
        graph.clear()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        merged["e2e"] = e2e(args, dev)
        print(json.dumps(merged["e2e"]))
    out.write_text(json.dumps(merged, indent=2) + "\n")


if __name__ == "__main__":
    main()
