"""Norm backward (norm.hip) at the hidden sizes that select each
register-chunk instantiation of norm_bwd_kernel (H / 2048 = 2, 4, 8 for
RMSNorm, plain and fused with the residual add; 1, 2, 4 and the scalar
fallback for LayerNorm) and at more rows than the grid has blocks.

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


# H = 2056 / 4104: the last occupied chunk is one thread's 8 columns (and
# the fourth chunk of 4104 is empty); 8192: the last H on the vector path;
# 8200: the scalar fallback; 768 at 2100 rows: a block folds several rows.
LN_SHAPES = [(5, 2056), (3, 4104), (2, 8192), (2100, 768), (2, 8200)]


@pytest.mark.parametrize("shape", LN_SHAPES)
def test_layernorm_bwd_chunks(shape):
    """dx, dw and db against F.layer_norm in f32 on the same bf16 inputs,
    each 2048-column chunk on its own so that an error confined to one
    chunk is not diluted by the others.  The outputs are bf16, so the
    expected error is one rounding (about 4e-3); the bound is the norm
    backward bound used throughout (3e-2)."""
    H = shape[-1]
    x = _rand(shape, 8) * 2
    w = 1 + _rand((H,), 9) * 0.1
    b = _rand((H,), 10) * 0.1
    dy = _rand(shape, 11)
    _, mu, rstd = ext().layernorm_fwd(x, w, b, 1e-5)
    dx, dw, db = ext().layernorm_bwd(dy, x, w, mu, rstd)

    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    br = b.float().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (H,), wr, br, 1e-5).backward(
        dy.float())
    for c0 in range(0, H, 2048):
        sl = slice(c0, min(c0 + 2048, H))
        errs = dict(dx=_rel_err(dx[..., sl], xr.grad[..., sl]),
                    dw=_rel_err(dw[sl], wr.grad[sl]),
                    db=_rel_err(db[sl], br.grad[sl]))
        print(shape, "columns", sl.start, sl.stop, errs)
        for k, e in errs.items():
            assert e < 3e-2, (k, sl, errs)

    dx2, dw2, db2 = ext().layernorm_bwd(dy, x, w, mu, rstd)
    assert torch.equal(dx, dx2)
    assert torch.equal(dw, dw2)
    assert torch.equal(db, db2)
