"""Mixture of experts on the CPU: the eager paths of ops/moe.py against the
fp64 references and bounds the GPU kernels are held to (tests/utils_moe.py),
and the qwen3-moe-debug model through build, backward and the trainer."""
import re

import pytest
import torch

from distributed_training_guide_amd.models import build_model, get_config
from distributed_training_guide_amd.models.llama import LlamaMLP, LlamaMoE
from distributed_training_guide_amd.ops import (moe_combine,
                                                moe_dispatch_index, moe_mlp,
                                                moe_router, moe_scatter)
from utils_moe import (MLP_SHAPE, ROUTER_RECIPES, ROUTER_SHAPES, ROW_CASES,
                       assert_router_close, assert_rows_close, index_cases,
                       index_ref, mlp_inputs, mlp_ref64, mlp_run,
                       router_logits, router_ref64, rows_inputs, rows_ref64)


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("recipe", ROUTER_RECIPES)
@pytest.mark.parametrize("shape", ROUTER_SHAPES)
def test_router_eager_within_bounds(shape, recipe, norm):
    T, E, k = shape
    logits, dw = router_logits(T, E, k, recipe, "cpu")
    logits.requires_grad_()
    idx, w = moe_router(logits, k, norm)
    (w * dw).sum().backward()
    if recipe == "masked":
        assert not (idx == 1).any()
    assert_router_close(idx, w.detach(), logits.grad,
                        router_ref64(logits.detach(), k, norm, dw),
                        f"{shape} {recipe} norm={norm}")


@pytest.mark.parametrize("T", [1, 70, 4099])
def test_dispatch_index_eager(T):
    for name, idx, E in index_cases(T):
        dest, offs = moe_dispatch_index(idx, E)
        rdest, roffs = index_ref(idx, E)
        assert torch.equal(dest, rdest) and torch.equal(offs, roffs), name
        # a permutation whose rows, read in order, are sorted by expert
        order = torch.empty_like(dest).long()
        order[dest.long()] = torch.arange(dest.numel())
        sorted_e = idx.reshape(-1)[order]
        assert (sorted_e[1:] >= sorted_e[:-1]).all(), name
        assert int(offs[-1]) == dest.numel(), name


@pytest.mark.parametrize("H,k,T", ROW_CASES)
def test_row_movers_eager_within_bounds(H, k, T):
    inp = rows_inputs(H, k, T, "cpu")
    x = inp["x"].clone().requires_grad_()
    yp = inp["yp"].clone().requires_grad_()
    w = inp["w"].clone().requires_grad_()
    xp = moe_scatter(x, inp["dest"], inp["k"])
    xp.backward(inp["dxp"])
    y = moe_combine(yp, inp["dest"], w)
    y.backward(inp["dy"])
    assert_rows_close(xp.detach(), y.detach(), x.grad, yp.grad, w.grad, inp,
                      rows_ref64(inp), f"H={H} k={k} T={T}")


def test_moe_mlp_eager_close_to_fp64():
    inp = mlp_inputs("cpu")
    got = mlp_run(moe_mlp, inp, MLP_SHAPE["k"], True)
    ref = mlp_ref64(inp, MLP_SHAPE["k"], True)
    for name, a, b in zip(("y", "dx", "drouter", "dgate_up", "ddown"),
                          got, ref):
        # three bf16 GEMM roundings deep: a few bf16 ulps of the largest
        # element
        assert (a - b).abs().max() <= 2.0 ** -5 * b.abs().max(), name


def test_debug_model_builds_and_trains_one_step():
    cfg = get_config("qwen3-moe-debug")
    assert cfg.num_experts == 8 and cfg.num_experts_per_tok == 2
    torch.manual_seed(0)
    model = build_model(cfg)
    assert all(isinstance(l.mlp, LlamaMoE) for l in model.layers)
    assert sum(p.numel() for p in model.parameters()) == cfg.num_parameters()
    ids = torch.randint(0, cfg.vocab_size, (2, 32))
    model(input_ids=ids, labels=ids).loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.layers[0].mlp.router.weight.grad.abs().sum() > 0


@pytest.mark.parametrize("name,params", [("qwen3-30b-a3b", 30.5e9),
                                         ("Qwen/Qwen3-235B-A22B", 235e9)])
def test_registry_sizes(name, params):
    cfg = get_config(name)
    assert cfg.num_experts == 128 and cfg.num_experts_per_tok == 8
    assert cfg.qk_norm and cfg.head_dim == 128 and cfg.norm_topk_prob
    assert abs(cfg.num_parameters() - params) < 0.01 * params


def test_dense_config_keeps_llama_mlp():
    model = build_model("qwen3-debug")
    assert all(type(l.mlp) is LlamaMLP for l in model.layers)


def test_fp8_conversion_leaves_the_moe_layer_alone():
    import dataclasses

    from distributed_training_guide_amd.trainer import apply_fp8

    # 16 experts: the router's 256 -> 16 would be eligible by shape
    cfg = dataclasses.replace(get_config("qwen3-moe-debug"), num_experts=16)
    model = build_model(cfg)
    names = apply_fp8(model)
    assert names and not any("router" in n or "mlp" in n for n in names)
    assert type(model.layers[0].mlp.router) is torch.nn.Linear


def test_expert_mm_rejects_bad_arguments_without_switching_paths():
    from distributed_training_guide_amd.ops import moe

    a, w = torch.randn(6, 16).bfloat16(), torch.randn(2, 8, 16).bfloat16()
    with pytest.raises(ValueError, match="expert_mm"):
        moe.expert_mm(a, w, torch.tensor([3, 6, 6], dtype=torch.int32))
    moe.expert_mm(a, w, torch.tensor([3, 6], dtype=torch.int32))
    assert moe.last_expert_mm_path == "grouped"


def test_tp_rejects_moe_config():
    from distributed_training_guide_amd.parallel.tp import TPLlamaForCausalLM

    with pytest.raises(ValueError, match="mixture-of-experts"):
        TPLlamaForCausalLM(get_config("qwen3-moe-debug"), mesh=None)


def test_trainer_lowers_loss_on_debug_model(tmp_path, capfd):
    from distributed_training_guide_amd.parallel.single import \
        SingleDeviceStrategy
    from distributed_training_guide_amd.trainer import (get_parser,
                                                        run_training)

    torch.manual_seed(0)
    args = get_parser().parse_args([
        "-m", "qwen3-moe-debug", "-d", "synthetic", "-s", "64", "-b", "2",
        "--num-samples", "2", "--num-workers", "0", "--log-freq", "1",
        "--save-dir", str(tmp_path), "--num-epochs", "6", "--max-steps", "6",
        "--device", "cpu", "--lr", "1e-3"])
    state = run_training(args, SingleDeviceStrategy(args))
    assert state["global_step"] == 6
    losses = [float(x) for x in re.findall(
        r"'running_loss': ([^,]+),", capfd.readouterr().err)]
    assert len(losses) == 6 and losses[-1] < losses[0], losses
