"""The norm bindings' argument checks (bindings.cpp: norm_check) and their
behaviour on zero rows.

A malformed call raises before anything is launched: a short weight would be
an out-of-bounds read, a wrong rstd / mu a read of the wrong bytes.  The
well-formed call beside each malformed one passes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_training_guide_amd._ext import ext

ROWS, H = 6, 64


def _bf(*shape):
    return torch.randn(*shape, device="cuda").bfloat16()


@pytest.fixture(scope="module")
def t():
    """Well-formed arguments of all six entry points, made once."""
    torch.manual_seed(0)
    d = dict(x=_bf(ROWS, H), w=_bf(H), b=_bf(H), dy=_bf(ROWS, H),
             dres=_bf(ROWS, H), delta=_bf(ROWS, H))
    d["rstd"] = ext().rmsnorm_fwd(d["x"], d["w"], 1e-5)[1]
    _, d["mu"], d["ln_rstd"] = ext().layernorm_fwd(d["x"], d["w"], d["b"],
                                                   1e-5)
    _, d["res_out"], d["add_rstd"] = ext().add_rmsnorm_fwd(
        d["x"], d["delta"], d["w"], 1e-5)
    return d


def _calls(t):
    """name -> (function, well-formed argument dict) for the six bindings."""
    e = ext()
    return {
        "rmsnorm_fwd": (lambda a: e.rmsnorm_fwd(a["x"], a["w"], 1e-5), t),
        "rmsnorm_bwd": (lambda a: e.rmsnorm_bwd(a["dy"], a["x"], a["w"],
                                                a["rstd"]), t),
        "add_rmsnorm_fwd": (lambda a: e.add_rmsnorm_fwd(
            a["x"], a["delta"], a["w"], 1e-5), t),
        "add_rmsnorm_bwd": (lambda a: e.add_rmsnorm_bwd(
            a["dy"], a["dres"], a["res_out"], a["w"], a["add_rstd"]), t),
        "layernorm_fwd": (lambda a: e.layernorm_fwd(a["x"], a["w"], a["b"],
                                                    1e-5), t),
        "layernorm_bwd": (lambda a: e.layernorm_bwd(
            a["dy"], a["x"], a["w"], a["mu"], a["ln_rstd"]), t),
    }


BAD = [
    # (entry point, argument replaced, how)
    ("rmsnorm_fwd", "w", lambda v: v[:H - 8].contiguous()),
    ("rmsnorm_bwd", "w", lambda v: v[:H - 8].contiguous()),
    ("add_rmsnorm_fwd", "w", lambda v: v[:H - 8].contiguous()),
    ("add_rmsnorm_bwd", "w", lambda v: v[:H - 8].contiguous()),
    ("layernorm_fwd", "w", lambda v: v[:H - 8].contiguous()),
    ("layernorm_bwd", "w", lambda v: v[:H - 8].contiguous()),
    ("layernorm_fwd", "b", lambda v: torch.cat([v, v[:8]])),
    ("rmsnorm_bwd", "dy", lambda v: v[:-1].contiguous()),
    ("add_rmsnorm_bwd", "dy", lambda v: v[:-1].contiguous()),
    ("add_rmsnorm_bwd", "dres", lambda v: v[:-1].contiguous()),
    ("add_rmsnorm_fwd", "delta", lambda v: v[:-1].contiguous()),
    ("layernorm_bwd", "dy", lambda v: v[:-1].contiguous()),
    ("rmsnorm_bwd", "rstd", lambda v: v.double()),
    ("add_rmsnorm_bwd", "add_rstd", lambda v: v.double()),
    ("layernorm_bwd", "ln_rstd", lambda v: v.double()),
    ("rmsnorm_bwd", "rstd", lambda v: v[:-1].contiguous()),
    ("layernorm_bwd", "ln_rstd", lambda v: v[:-1].contiguous()),
    ("layernorm_bwd", "mu", lambda v: v[:-1].contiguous()),
    ("layernorm_bwd", "mu", lambda v: v.cpu()),
    ("rmsnorm_fwd", "x", lambda v: v.t().contiguous().t()),
    ("rmsnorm_bwd", "x", lambda v: v.t().contiguous().t()),
    ("layernorm_fwd", "x", lambda v: v.t().contiguous().t()),
    ("layernorm_bwd", "x", lambda v: v.t().contiguous().t()),
    ("add_rmsnorm_fwd", "x", lambda v: v.t().contiguous().t()),
]


@pytest.mark.parametrize("name,arg,how", BAD,
                         ids=[f"{n}-{a}-{i}" for i, (n, a, _) in
                              enumerate(BAD)])
def test_malformed_argument_raises(t, name, arg, how):
    fn, good = _calls(t)[name]
    fn(good)  # the well-formed call passes
    bad = dict(good)
    bad[arg] = how(good[arg])
    with pytest.raises(RuntimeError):
        fn(bad)
    torch.cuda.synchronize()


def test_add_rmsnorm_bwd_repeats_the_forward_H_check():
    e = ext()
    x, w = _bf(3, 100), _bf(100)
    rstd = e.rmsnorm_fwd(x, w, 1e-5)[1]
    e.rmsnorm_bwd(x, x, w, rstd)  # the plain backward takes H = 100
    with pytest.raises(RuntimeError):
        e.add_rmsnorm_fwd(x, x, w, 1e-5)
    with pytest.raises(RuntimeError):
        e.add_rmsnorm_bwd(x, x, x, w, rstd)
    torch.cuda.synchronize()


def test_zero_rows():
    e = ext()
    x = torch.empty(0, H, device="cuda", dtype=torch.bfloat16)
    w, b = _bf(H), _bf(H)

    y, rstd = e.rmsnorm_fwd(x, w, 1e-5)
    assert y.shape == x.shape and rstd.numel() == 0
    dx, dw = e.rmsnorm_bwd(x, x, w, rstd)
    assert dx.shape == x.shape
    assert dw.shape == w.shape and not dw.any()

    y, mu, rstd = e.layernorm_fwd(x, w, b, 1e-5)
    assert y.shape == x.shape and mu.numel() == 0 and rstd.numel() == 0
    dx, dw, db = e.layernorm_bwd(x, x, w, mu, rstd)
    assert dx.shape == x.shape
    assert dw.shape == w.shape and not dw.any()
    assert db.shape == w.shape and not db.any()

    torch.cuda.synchronize()
    x3 = _bf(3, H)
    y3, rstd3 = e.rmsnorm_fwd(x3, w, 1e-5)
    e.rmsnorm_bwd(x3, x3, w, rstd3)
    torch.cuda.synchronize()
    assert torch.isfinite(y3.float()).all()
