"""Attention kernels specialised on the head dim (D = 64 / 128 template
instantiations) and their raw-exp2 softmax, against the fp32 reference.

Small shapes at which a specialised kernel can go wrong: under one tile,
ragged, several tiles with GQA, eight (batch, kv-head) groups of several
blocks (the XCD-aware block remap); each with and without the document mask.
Then the edges of the raw hardware exp2: scores of about +-200 (underflow to
0, saturated rows) and a document layout whose 16-row groups meet fully
masked diagonal tiles.

Bounds are the project's own (tests/test_ops_gpu.py): relative Frobenius
error 3e-2 for o, 5e-2 for dq / dk / dv."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_training_guide_amd import ops
from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops import reference as R

# name: (B, S, Hq, Hkv, document lengths of every batch row)
SHAPES = {
    "under_tile": (1, 48, 2, 2, [5, 43]),
    "ragged": (1, 200, 2, 2, [77, 123]),
    "tiles_gqa": (2, 256, 8, 2, [1, 62, 1, 70, 122]),
    # B * Hkv = 8 groups with four forward / dq blocks (GQA 2 x 2 q tiles)
    # and four dkdv blocks each: the XCD-aware remap takes its
    # groups-divide-over-the-XCDs branch and is not the identity, so a wrong
    # remap computes the wrong (b, h, tile)
    "remap_xcd": (2, 256, 8, 4, [1, 62, 1, 70, 122]),
}


def _doc_start(lens, B, S):
    assert sum(lens) == S
    start = torch.zeros(S, dtype=torch.int32)
    at = 0
    for n in lens:
        start[at:at + n] = at
        at += n
    return start.repeat(B, 1).cuda()


def _rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _run(q, k, v, dout, start, scale):
    """The extension called directly, and the fp32 reference with its
    gradients: ((o, dq, dk, dv), (o, dq, dk, dv))."""
    if start is None:
        o, lse = ext().attn_fwd(q, k, v, scale)
        dq, dk, dv = ext().attn_bwd(dout, q, k, v, o, lse, scale)
    else:
        ops.validate_doc_start(start)
        bounds = ops.doc_bounds(start)
        o, lse = ext().attn_fwd_doc(q, k, v, bounds.start, scale)
        dq, dk, dv = ext().attn_bwd_doc(dout, q, k, v, o, lse, bounds.start,
                                        bounds.end, scale)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    oref = R.attention_ref(qr, kr, vr, scale, doc_start=start)
    oref.backward(dout.float())
    return (o, dq, dk, dv), (oref.detach(), qr.grad, kr.grad, vr.grad)


def _check(got, ref, tag):
    errs = {n: _rel_err(a, b)
            for n, a, b in zip(("o", "dq", "dk", "dv"), got, ref)}
    print(tag, {n: f"{e:.3e}" for n, e in errs.items()})
    for n, a in zip(errs, got):
        assert torch.isfinite(a.float()).all(), (tag, n)
    assert errs["o"] < 3e-2, errs
    assert errs["dq"] < 5e-2, errs
    assert errs["dk"] < 5e-2, errs
    assert errs["dv"] < 5e-2, errs


@pytest.mark.parametrize("doc", [False, True], ids=["causal", "doc"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name", list(SHAPES))
def test_matches_reference(name, D, doc):
    B, S, Hq, Hkv, lens = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g).bfloat16()

    q, k, v = rnd(B, S, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
    dout = rnd(B, S, Hq, D)
    start = _doc_start(lens, B, S) if doc else None
    got, ref = _run(q, k, v, dout, start, 1 / math.sqrt(D))
    _check(got, ref, (name, D, doc))


# ---- raw exp2: large scores and fully masked diagonal tiles ----
# D=128, S=192, B=1, Hq=Hkv=2.  q and k are scaled by 6.9: a score is
# scale * q.k with q.k a sum of 128 products of two N(0, 6.9^2) values,
# standard deviation 6.9^2 * sqrt(128) / sqrt(128) = 47.6, so over the
# 2 * 192 * 192 / 2 = 37k visible scores the extremes reach about
# +-4.2 sigma = +-200, and within a long row the scores span some 250 (x
# log2(e) = 360 in exp2's argument, far below the 2^-126 where the raw
# instruction returns 0): most p underflow to exactly 0 and each row is
# carried by one or two keys.
#
# The layout [70, 122] starts the second document at row 70, inside the
# 16-row group 64..79 (wave 0's second group of q tile 0) and inside K/V
# tile 1: rows 70..79 see no key of tile 0, which the kernels still visit
# for rows 64..69 — a tile that is fully masked for those rows while their
# running max is still -inf.  Rows 128..191 (q tile 1) start at tile 1.
_EDGE_LENS = [70, 122]


@functools.lru_cache(maxsize=None)
def _edge_case(doc):
    B, S, H, D = 1, 192, 2, 128
    g = torch.Generator(device="cuda").manual_seed(7)

    def rnd(*shape, mul=1.0):
        return (mul * torch.randn(*shape, device="cuda",
                                  generator=g)).bfloat16()

    q, k = rnd(B, S, H, D, mul=6.9), rnd(B, S, H, D, mul=6.9)
    v, dout = rnd(B, S, H, D), rnd(B, S, H, D)
    start = _doc_start(_EDGE_LENS, B, S) if doc else None
    scale = 1 / math.sqrt(D)
    kk = k.float().permute(0, 2, 1, 3)
    s = scale * (q.float().permute(0, 2, 1, 3) @ kk.transpose(-1, -2))
    vis = torch.ones(S, S, dtype=torch.bool, device="cuda").tril()
    peak = s.masked_fill(~vis, 0).abs().max().item()
    span = (s.masked_fill(~vis, -1e30).amax(-1)
            - s.masked_fill(~vis, 1e30).amin(-1)).max().item()
    return (q, k, v, dout, start, scale), (peak, span), \
        _run(q, k, v, dout, start, scale)


@pytest.mark.parametrize("doc", [False, True], ids=["causal", "doc"])
def test_large_scores_stay_finite_and_accurate(doc):
    _, (peak, span), (got, ref) = _edge_case(doc)
    print("largest |score|", peak, "largest in-row span", span)
    # the inputs are what the comment above says: 3.2 sigma is passed by one
    # score in 700, and 128 / log2(e) = 89 already underflows exp2
    assert peak > 150 and span > 150
    _check(got, ref, ("edge", doc))


@pytest.mark.parametrize("doc", [False, True], ids=["causal", "doc"])
def test_first_row_of_a_document_returns_its_value(doc):
    """A row that sees one key has p = exp2(0) = 1: o is that key's v, to
    the bf16 rounding of the stored output (v is bf16 already: exact)."""
    (q, k, v, dout, start, scale), _, ((o, *_), _) = _edge_case(doc)
    rows = [0] + ([_EDGE_LENS[0]] if doc else [])
    for r in rows:
        assert torch.equal(o[:, r], v[:, r]), r


@pytest.mark.parametrize("doc", [False, True], ids=["causal", "doc"])
def test_backward_bindings_reject_bad_inputs(doc):
    """attn_bwd / attn_bwd_doc check their tensors like the forward does and
    raise before any launch: a head dim without an instantiation, and a q
    that is not contiguous."""
    B, S, H = 1, 64, 2
    start = _doc_start([S], B, S)
    bounds = ops.doc_bounds(start)

    def bwd(dout, q, k, v, o, lse):
        if doc:
            return ext().attn_bwd_doc(dout, q, k, v, o, lse, bounds.start,
                                      bounds.end, 0.125)
        return ext().attn_bwd(dout, q, k, v, o, lse, 0.125)

    def inputs(D):
        t = [torch.zeros(B, S, H, D, device="cuda", dtype=torch.bfloat16)
             for _ in range(5)]
        return t + [torch.zeros(B, H, S, device="cuda")]

    with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
        bwd(*inputs(96))
    dout, q, k, v, o, lse = inputs(64)
    q_nc = torch.zeros(B, S, 64, H, device="cuda",
                       dtype=torch.bfloat16).transpose(2, 3)
    assert q_nc.shape == q.shape and not q_nc.is_contiguous()
    with pytest.raises(RuntimeError, match="q must be contiguous"):
        bwd(dout, q_nc, k, v, o, lse)
    torch.cuda.synchronize()
