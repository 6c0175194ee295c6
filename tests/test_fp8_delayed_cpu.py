"""FP8 delayed scaling (ops.fp8_linear.Fp8DelayedState) through the eager
path: the amax history, and the stationary-input identity with the dynamic
recipe.  Every check is an equality.  `check_history` takes the device, so
tests/test_fp8_delayed_gpu.py runs the same sequence through the kernels."""
import pytest
import torch

from distributed_training_guide_amd.models import build_model
from distributed_training_guide_amd.ops import (Fp8DelayedState,
                                                convert_linears_to_fp8,
                                                fp8_linear, fp8_quantize,
                                                fp8_swiglu_linear, silu_mul)
from distributed_training_guide_amd.ops.fp8_linear import (_cast_ref,
                                                           _scales_ref)

MNK = [(16, 16, 16), (80, 48, 208), (256, 192, 128)]
# rising, a spike that leaves the window of 4 after 4 calls, falling
AMAXES = [1.0, 2.0, 3.0, 64.0, 2.5, 2.0, 1.5, 1.0, 0.5, 0.25]


def _bytes(t):
    return t.view(torch.uint8).cpu()


def check_history(device):
    state = Fp8DelayedState(history=4)
    g = torch.Generator().manual_seed(0)
    top = torch.tensor(448.0)
    before = None  # the pair current before the call
    for i, amax in enumerate(AMAXES):
        x = ((torch.rand(80, 48, generator=g) - 0.5) * amax).bfloat16()
        x[79, 47] = -amax
        if before is None:
            before = _scales_ref(x)
        q, qt, scale, inv = fp8_quantize(x.to(device), True, True,
                                         state=state, role="x")
        assert scale.cpu() == before[0] and inv.cpu() == before[1], i
        ref = _cast_ref(x, before[0])
        assert torch.equal(_bytes(q), _bytes(ref)), i
        assert torch.equal(_bytes(qt), _bytes(ref.t().contiguous())), i
        m = torch.tensor(max(AMAXES[max(0, i - 3):i + 1]))
        before = (top / m, m / top)
        pair = state.role("x").pair
        assert pair[0].cpu() == before[0] and pair[1].cpu() == before[1], i
    # a NaN: visible in this call's output, absent from the next pair
    x[5, 7] = float("nan")
    q = fp8_quantize(x.to(device), state=state, role="x")[0]
    assert torch.equal(q.float().isnan().cpu(), x.isnan())
    pair = state.role("x").pair
    assert pair[0].cpu() == before[0] and pair[1].cpu() == before[1]
    assert torch.isfinite(state.role("x").history).all()


def _fwd_bwd(fn, a, w, dy):
    a, w = a.clone().requires_grad_(), w.clone().requires_grad_()
    y = fn(a, w)
    y.backward(dy)
    return y.detach(), a.grad, w.grad


def check_stationary(device, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16().to(device)
    w = (0.02 * torch.randn(N, K, generator=g)).bfloat16().to(device)
    dy = torch.randn(M, N, generator=g).bfloat16().to(device)
    state = Fp8DelayedState()
    for _ in range(2):
        got = _fwd_bwd(lambda a, b: fp8_linear(a, b, state), x, w, dy)
    for a, b in zip(got, _fwd_bwd(fp8_linear, x, w, dy)):
        assert torch.equal(a, b)


def check_swiglu_linear(device, M, N, I):
    g = torch.Generator().manual_seed(M + N + I)
    gu = torch.randn(M, 2 * I, generator=g).bfloat16().to(device)
    w = (0.02 * torch.randn(N, I, generator=g)).bfloat16().to(device)
    dy = torch.randn(M, N, generator=g).bfloat16().to(device)
    fused, plain = Fp8DelayedState(), Fp8DelayedState()
    for _ in range(2):
        got = _fwd_bwd(lambda a, b: fp8_swiglu_linear(a, b, fused), gu, w, dy)
        ref = _fwd_bwd(lambda a, b: fp8_linear(silu_mul(a), b, plain), gu, w,
                       dy)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_history_eager():
    check_history("cpu")


@pytest.mark.parametrize("M,N,K", MNK)
def test_stationary_input_equals_dynamic_eager(M, N, K):
    check_stationary("cpu", M, N, K)


def test_swiglu_linear_equals_composition_eager():
    check_swiglu_linear("cpu", 80, 48, 208)


def test_convert_delayed_keeps_state_dict_and_default_recipe():
    model = build_model("llama-debug", device="cpu", dtype=torch.bfloat16)
    keys = list(model.state_dict().keys())
    names = convert_linears_to_fp8(model, recipe="delayed", history=8)
    assert list(model.state_dict().keys()) == keys
    mods = dict(model.named_modules())
    assert all(mods[n].fp8_state.history == 8 for n in names)
    other = build_model("llama-debug", device="cpu", dtype=torch.bfloat16)
    convert_linears_to_fp8(other)
    assert all(m.fp8_state is None for m in other.modules()
               if hasattr(m, "fp8_state"))
    with pytest.raises(ValueError, match="recipe"):
        convert_linears_to_fp8(other, recipe="static")
