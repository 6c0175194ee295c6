"""moe_router.hip and moe_dispatch.hip on the GPU: every output per element
against fp64 (references and bounds in tests/utils_moe.py, shown to hold for
the eager paths in tests/test_moe_cpu.py), exact selection and layout,
run-to-run equality of the backward, and the composed layer against the
torch-op chain."""
import pytest
import torch

from distributed_training_guide_amd.ops import (moe_combine,
                                                moe_dispatch_index, moe_mlp,
                                                moe_router, moe_scatter)
from distributed_training_guide_amd.ops import moe as moe_ops
from utils_moe import (MLP_SHAPE, ROUTER_RECIPES, ROUTER_SHAPES, ROW_CASES,
                       assert_router_close, assert_rows_close, index_cases,
                       index_ref, mlp_inputs, mlp_ref64, mlp_run,
                       router_logits, router_ref64, rows_inputs, rows_ref64)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("recipe", ROUTER_RECIPES)
@pytest.mark.parametrize("shape", ROUTER_SHAPES)
def test_router_matches_fp64(shape, recipe, norm):
    T, E, k = shape
    logits, dw = router_logits(T, E, k, recipe, "cuda")
    logits.requires_grad_()
    idx, w = moe_router(logits, k, norm)
    (w * dw).sum().backward()
    if recipe == "masked":
        assert not (idx == 1).any()
    ref = router_ref64(logits.detach(), k, norm, dw)
    assert_router_close(idx, w.detach(), logits.grad, ref,
                        f"{shape} {recipe} norm={norm}")


@pytest.mark.parametrize("T", [1, 70, 4099])
def test_dispatch_index_is_the_stable_sort(T):
    for name, idx, E in index_cases(T):
        dest, offs = moe_dispatch_index(idx.cuda(), E)
        rdest, roffs = index_ref(idx, E)
        assert dest.dtype == offs.dtype == torch.int32
        assert torch.equal(dest.cpu(), rdest), f"T={T} {name} dest"
        assert torch.equal(offs.cpu(), roffs), f"T={T} {name} offs"


def _row_movers(inp):
    x = inp["x"].clone().requires_grad_()
    yp = inp["yp"].clone().requires_grad_()
    w = inp["w"].clone().requires_grad_()
    xp = moe_scatter(x, inp["dest"], inp["k"])
    xp.backward(inp["dxp"])
    y = moe_combine(yp, inp["dest"], w)
    y.backward(inp["dy"])
    return xp.detach(), y.detach(), x.grad, yp.grad, w.grad


@pytest.mark.parametrize("H,k,T", ROW_CASES)
def test_row_movers_match_fp64_and_repeat(H, k, T):
    inp = rows_inputs(H, k, T, "cuda")
    first = _row_movers(inp)
    assert_rows_close(*first, inp, rows_ref64(inp), f"H={H} k={k} T={T}")
    for a, b in zip(first, _row_movers(inp)):
        assert torch.equal(a, b)


def test_moe_mlp_against_torch_chain():
    """The fused layer may err against fp64 at most twice as much as the
    torch-op chain on the same device (stable sort, index_select, the same
    GEMM helper, index_add_ in f32), per tensor: both round at the same
    three GEMM outputs and differ only in accumulation order."""
    inp = mlp_inputs("cuda")
    k = MLP_SHAPE["k"]
    ref = mlp_ref64(inp, k, True)
    fused = mlp_run(moe_mlp, inp, k, True)
    chain = mlp_run(moe_ops.moe_mlp_eager, inp, k, True)
    print("expert GEMM path:", moe_ops.last_expert_mm_path)
    names = ("y", "dx", "drouter", "dgate_up", "ddown")
    errs = [((f - r).abs().max().item(), (c - r).abs().max().item())
            for f, c, r in zip(fused, chain, ref)]
    for name, (ef, ec) in zip(names, errs):
        print(f"{name}: fused {ef:.4e} chain {ec:.4e}")
    for name, (ef, ec) in zip(names, errs):
        assert ef <= 2.0 * ec, (name, ef, ec)
