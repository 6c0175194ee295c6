"""RMSNorm backward at the hidden sizes that select each register-chunk
instantiation of rmsnorm_bwd_kernel (H / 2048 = 2, 4, 8) and at more rows
than the grid has blocks, plain and fused with the residual add.

Bounds are those of tests/test_ops_gpu.py (relative Frobenius error 3e-2).
dw comes from per-block partials folded in a fixed order, with no atomics:
two calls on the same inputs agree to the last bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_training_guide_amd import ops
from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops import reference as R
from distributed_training_guide_amd.ops.rmsnorm import add_rmsnorm

SHAPES = [(12, 4096), (5, 8192), (3, 16384), (2100, 4096)]


def _rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _rand(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g).bfloat16()


@pytest.mark.parametrize("shape", SHAPES)
def test_rmsnorm_bwd(shape):
    x = _rand(shape, 0).requires_grad_(True)
    w = _rand(shape[-1:], 1).requires_grad_(True)
    dy = _rand(shape, 2)
    y = ops.rmsnorm(x, w, 1e-5)
    y.backward(dy)
    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    R.rmsnorm_ref(xr, wr, 1e-5).backward(dy.float())
    errs = dict(dx=_rel_err(x.grad, xr.grad), dw=_rel_err(w.grad, wr.grad))
    print(shape, errs)
    assert errs["dx"] < 3e-2, errs
    assert errs["dw"] < 3e-2, errs

    rstd = ext().rmsnorm_fwd(x.detach(), w.detach(), 1e-5)[1]
    dx1, dw1 = ext().rmsnorm_bwd(dy, x.detach(), w.detach(), rstd)
    dx2, dw2 = ext().rmsnorm_bwd(dy, x.detach(), w.detach(), rstd)
    assert torch.equal(dw1, dw2)
    assert torch.equal(dx1, dx2)
    assert torch.equal(dw1, w.grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_add_rmsnorm_bwd(shape):
    res = _rand(shape, 3).requires_grad_(True)
    delta = _rand(shape, 4).requires_grad_(True)
    w = _rand(shape[-1:], 5).requires_grad_(True)
    dy, dres = _rand(shape, 6), _rand(shape, 7)
    y, res_out = add_rmsnorm(res, delta, w, 1e-5)
    torch.autograd.backward([y, res_out], [dy, dres])
    # the norm is taken of the bf16-rounded sum that res_out stores
    sr = res_out.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    yr = R.rmsnorm_ref(sr, wr, 1e-5)
    torch.autograd.backward([yr, sr], [dy.float(), dres.float()])
    errs = dict(dres=_rel_err(res.grad, sr.grad),
                ddelta=_rel_err(delta.grad, sr.grad),
                dw=_rel_err(w.grad, wr.grad))
    print(shape, errs)
    assert errs["dres"] < 3e-2, errs
    assert errs["ddelta"] < 3e-2, errs
    assert errs["dw"] < 3e-2, errs

    _, ro, rstd = ext().add_rmsnorm_fwd(res.detach(), delta.detach(),
                                        w.detach(), 1e-5)
    args = (dy, dres, ro, w.detach(), rstd)
    dx1, dw1 = ext().add_rmsnorm_bwd(*args)
    dx2, dw2 = ext().add_rmsnorm_bwd(*args)
    assert torch.equal(dw1, dw2)
    assert torch.equal(dx1, dx2)
    assert torch.equal(dw1, w.grad)
