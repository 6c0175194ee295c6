"""FP8 delayed scaling on the GPU (fp8_delayed.hip): the one-pass cast with
amax against torch's CPU cast and the two-pass kernels, the history kernel,
the stationary-input identity with the dynamic recipe, SwiGLU written as
e4m3 against the unfused chain, and llama-debug under recipe="delayed".
Every check is an equality: the kernels are defined bit for bit."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_fp8_delayed_cpu as eager
from distributed_training_guide_amd.models import build_model
from distributed_training_guide_amd.ops import (Fp8DelayedState,
                                                convert_linears_to_fp8,
                                                fp8_quantize, silu_mul)
from distributed_training_guide_amd.ops.fp8_linear import _cast_ref

# the module: `ops.fp8_linear` itself names the function of that name
fp8_mod = importlib.import_module(
    "distributed_training_guide_amd.ops.fp8_linear")

# one patch, one full tile, tiles hanging over both edges, many tiles along
# each axis (more than 1024 partials / a vector tail in the fold)
SHAPES = [(16, 16), (64, 64), (80, 48), (208, 4112), (4112, 80)]


def _state_at(scale):
    """A state whose role `x` is seeded with `scale` and a history of one
    slot, which then holds exactly the last call's amax."""
    state = Fp8DelayedState(history=1)
    r = state.role("x", scale.device)
    r.pair, r.seeded = (scale, scale), True
    return state


@pytest.mark.parametrize("rowwise,transposed",
                         [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("R,C", SHAPES)
def test_cast_with_amax(R, C, rowwise, transposed):
    g = torch.Generator().manual_seed(R * 7 + C)
    x = torch.randn(R, C, generator=g).bfloat16()
    x[R - 1, C - 1] = -37.0  # the amax sits in the last (ragged) tile
    scale = torch.tensor(448.0 / 3.0)  # |x| > 3 overflows: the clamp works
    xg, sg = x.cuda(), scale.cuda()
    state = _state_at(sg)
    q, qt, _, _ = fp8_quantize(xg, rowwise, transposed, state=state, role="x")
    q2, qt2, _, _ = fp8_quantize(xg, rowwise, transposed, scale=sg)
    ref = _cast_ref(x, scale)
    assert (ref.float().abs() == 448).any()
    if rowwise:
        assert torch.equal(eager._bytes(q), eager._bytes(ref))
        assert torch.equal(q.view(torch.uint8), q2.view(torch.uint8))
    if transposed:
        assert torch.equal(eager._bytes(qt), eager._bytes(ref.t().contiguous()))
        assert torch.equal(qt.view(torch.uint8), qt2.view(torch.uint8))
    assert state.role("x").history.item() == 37.0 == x.abs().max().item()


def test_history():
    eager.check_history("cuda")


@pytest.mark.parametrize("M,N,K", eager.MNK)
def test_stationary_input_equals_dynamic(M, N, K):
    eager.check_stationary("cuda", M, N, K)


@pytest.mark.parametrize("R,I", [(16, 16), (80, 48), (208, 4112)])
def test_silu_mul_fp8_equals_unfused_chain(R, I):
    g = torch.Generator().manual_seed(R + I)
    gu = (2.0 * torch.randn(R, 2 * I, generator=g)).bfloat16().cuda()
    h = silu_mul(gu)
    scale = (torch.tensor(448.0) / h.abs().max().float().cpu() * 2).cuda()
    state = _state_at(scale)
    hq, hqt, _, _, path = state.swiglu(gu)
    q, qt, _, _ = fp8_quantize(h, True, True, scale=scale)
    assert path == "fused"
    assert torch.equal(hq.view(torch.uint8), q.view(torch.uint8))
    assert torch.equal(hqt.view(torch.uint8), qt.view(torch.uint8))
    assert state.role("x").history.item() == h.abs().max().item()


@pytest.mark.parametrize("M,N,I", [(16, 16, 16), (80, 48, 208)])
def test_swiglu_linear_equals_composition(M, N, I):
    eager.check_swiglu_linear("cuda", M, N, I)
    assert fp8_mod.last_swiglu_path == "fused"


def test_llama_debug_delayed_three_steps():
    torch.manual_seed(0)
    model = build_model("llama-debug", device="cuda", dtype=torch.bfloat16)
    keys = list(model.state_dict().keys())
    convert_linears_to_fp8(model, recipe="delayed")
    assert list(model.state_dict().keys()) == keys
    ids = torch.randint(0, 1024, (2, 64), device="cuda")
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    for step in range(3):
        fp8_mod.last_swiglu_path = None
        loss = model(input_ids=ids, labels=ids).loss
        loss.backward()
        assert fp8_mod.last_swiglu_path == ("fused" if step else "seed")
        assert torch.isfinite(loss)
        for name, p in model.named_parameters():
            assert torch.isfinite(p.grad).all(), (step, name)
        opt.step()
        opt.zero_grad()
