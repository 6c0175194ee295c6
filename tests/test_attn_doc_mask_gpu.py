"""Document-masked causal attention kernels (attn_fwd_doc / attn_bwd_doc)
against the fp32 reference, plus the exact properties a norm cannot see:
one document == plain causal bitwise, every token its own document, and
bit-exact isolation of documents from each other.

Layouts are lists of document lengths; each one targets a boundary of the
128-row q tile, the 64-key tile, or the interleaved 16-row groups."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_training_guide_amd import ops
from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops import reference as R

# name: (B, S, Hq, Hkv, D, document lengths per batch row)
LAYOUTS = {
    # starts at 1, 63, 64, 134: length-1 documents, a boundary on a tile
    # edge and one either side of it
    "mid": (1, 256, 4, 4, 64, [[1, 62, 1, 70, 122]]),
    # q tiles at 256 and 384 start at K/V tile 3 (odd buffer parity); GQA
    "odd_t0": (1, 512, 8, 2, 128, [[200, 312]]),
    # start tile 2 (even parity)
    "even_t0": (1, 512, 4, 1, 128, [[130, 382]]),
    # dkdv block 0 walks only 2 q tiles; block 1 straddles two documents
    "early_end": (1, 512, 4, 4, 64, [[100, 412]]),
    "ragged": (1, 200, 2, 2, 128, [[77, 123]]),   # S not a tile multiple
    "small": (1, 48, 2, 2, 64, [[5, 43]]),        # S smaller than a tile
    # table indexing over b; tile-aligned boundaries
    "batch": (2, 256, 8, 2, 128, [[256], [64, 64, 128]]),
}


def _doc_start(lens, S):
    start = torch.zeros(len(lens), S, dtype=torch.int32)
    for b, ls in enumerate(lens):
        assert sum(ls) == S
        at = 0
        for n in ls:
            start[b, at:at + n] = at
            at += n
    return start.cuda()


def _inputs(name, seed=0):
    B, S, Hq, Hkv, D, lens = LAYOUTS[name]
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g).bfloat16()

    q, k, v = rnd(B, S, Hq, D), rnd(B, S, Hkv, D), rnd(B, S, Hkv, D)
    dout = rnd(B, S, Hq, D)
    return q, k, v, dout, _doc_start(lens, S), 1 / math.sqrt(D)


def _run_doc(q, k, v, dout, bounds, scale):
    """The extension called directly: (o, lse, dq, dk, dv)."""
    o, lse = ext().attn_fwd_doc(q, k, v, bounds.start, scale)
    dq, dk, dv = ext().attn_bwd_doc(dout, q, k, v, o, lse, bounds.start,
                                    bounds.end, scale)
    return o, lse, dq, dk, dv


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, kernel results and the fp32 reference of one layout, computed
    once and shared (read-only) by the tests below."""
    q, k, v, dout, start, scale = _inputs(name)
    bounds = ops.doc_bounds(start)
    ops.validate_doc_start(start)
    got = _run_doc(q, k, v, dout, bounds, scale)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    oref = R.attention_ref(qr, kr, vr, scale, doc_start=start)
    oref.backward(dout.float())
    ref = (oref.detach(), qr.grad, kr.grad, vr.grad)
    return (q, k, v, dout, bounds, scale), got, ref


def _rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _row_err(o, ref):
    """max over (b, s, h) rows of |o_row - ref_row| / (sqrt(D) rms(ref)): a
    single wrong row is not averaged away."""
    o = o.float()
    ref = ref.float()
    D = o.shape[-1]
    rms = ref.pow(2).mean().sqrt()
    return ((o - ref).norm(dim=-1).max() / (math.sqrt(D) * rms)).item()


# ---- 1. against the fp32 reference ----
# Bounds: the project's own from test_ops_gpu.py (relative Frobenius error
# 3e-2 forward, 5e-2 backward).  The per-row bound for o is 3e-2 as well:
# the unchanged causal path (doc=None) measures at most 1.1e-2 in this
# metric at these shapes (profiles/attn_doc_mask.json, "row_err_causal"),
# below the 1.5e-2 above which the bound would have to be widened.
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_matches_reference(name):
    _, (o, _lse, dq, dk, dv), (oref, dqr, dkr, dvr) = _case(name)
    errs = dict(o=_rel_err(o, oref), o_row=_row_err(o, oref),
                dq=_rel_err(dq, dqr), dk=_rel_err(dk, dkr),
                dv=_rel_err(dv, dvr))
    print(name, {k: f"{v:.3e}" for k, v in errs.items()})
    assert errs["o"] < 3e-2, errs
    assert errs["o_row"] < 3e-2, errs
    assert errs["dq"] < 5e-2, errs
    assert errs["dk"] < 5e-2, errs
    assert errs["dv"] < 5e-2, errs


# ---- 2. one document == plain causal, bitwise ----
@pytest.mark.parametrize("name", ["mid", "odd_t0"])
def test_single_document_is_plain_causal(name):
    q, k, v, dout, start, scale = _inputs(name)
    bounds = ops.doc_bounds(torch.zeros_like(start))
    o, lse, dq, dk, dv = _run_doc(q, k, v, dout, bounds, scale)
    o0, lse0 = ext().attn_fwd(q, k, v, scale)
    dq0, dk0, dv0 = ext().attn_bwd(dout, q, k, v, o0, lse0, scale)
    for what, a, b in (("o", o, o0), ("lse", lse, lse0), ("dq", dq, dq0),
                       ("dk", dk, dk0), ("dv", dv, dv0)):
        assert torch.equal(a, b), what
    # and through the public op
    qa = q.clone().requires_grad_(True)
    qb = q.clone().requires_grad_(True)
    oa = ops.flash_attention(qa, k, v, doc=bounds)
    ob = ops.flash_attention(qb, k, v)
    assert torch.equal(oa, ob)
    oa.backward(dout)
    ob.backward(dout)
    assert torch.equal(qa.grad, qb.grad)


# ---- 3. every token its own document ----
@pytest.mark.parametrize("name", ["small", "mid"])
def test_every_token_its_own_document(name):
    q, k, v, dout, start, scale = _inputs(name)
    B, S, Hq, D = q.shape
    group = Hq // k.shape[2]
    own = torch.arange(S, device="cuda", dtype=torch.int32).repeat(B, 1)
    o, lse = ext().attn_fwd_doc(q, k, v, own, scale)
    assert torch.equal(o, v.repeat_interleave(group, dim=2))
    kk = k.repeat_interleave(group, dim=2)
    want = scale * (q.float() * kk.float()).sum(-1)        # [B,S,Hq]
    # fp32 accumulation of D = 64 exact bf16 products in another order:
    # D * 2 eps * sum|q_d k_d| * scale ~ 64 * 1.2e-7 * 41 * 0.125 = 4e-5
    # even if every step truncates
    torch.testing.assert_close(lse, want.permute(0, 2, 1), rtol=1e-5,
                               atol=1e-4)


# ---- 4. exact isolation ----
@pytest.mark.parametrize("name", ["mid", "odd_t0"])
def test_documents_are_isolated_bitwise(name):
    (q, k, v, dout, bounds, scale), (o, lse, dq, dk, dv), _ = _case(name)
    nA = LAYOUTS[name][5][0][0]     # the first document
    g = torch.Generator(device="cuda").manual_seed(123)

    def noise(t):
        return (4 * torch.randn(t.shape, device="cuda",
                                generator=g)).bfloat16()

    # other keys/values inside A: nothing outside A may move
    k2, v2 = k.clone(), v.clone()
    k2[:, :nA] = noise(k[:, :nA])
    v2[:, :nA] = noise(v[:, :nA])
    o2, lse2, dq2, _, _ = _run_doc(q, k2, v2, dout, bounds, scale)
    assert not torch.equal(o2[:, :nA], o[:, :nA])       # A itself did change
    assert torch.equal(o2[:, nA:], o[:, nA:])
    assert torch.equal(lse2[:, :, nA:], lse[:, :, nA:])
    assert torch.equal(dq2[:, nA:], dq[:, nA:])

    # other queries/dout outside A: dk, dv on A's keys may not move
    q3, d3 = q.clone(), dout.clone()
    q3[:, nA:] = noise(q[:, nA:])
    d3[:, nA:] = noise(dout[:, nA:])
    _, _, _, dk3, dv3 = _run_doc(q3, k, v, d3, bounds, scale)
    assert not torch.equal(dk3[:, nA:], dk[:, nA:])
    assert torch.equal(dk3[:, :nA], dk[:, :nA])
    assert torch.equal(dv3[:, :nA], dv[:, :nA])


# ---- 5. autograd ----
def test_autograd_matches_extension():
    (q, k, v, dout, bounds, scale), (o, _lse, dq, dk, dv), _ = _case("batch")
    for doc in (bounds, bounds.start):      # DocBounds or raw doc_start
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        oa = ops.flash_attention(qa, ka, va, doc=doc)
        oa.backward(dout)
        assert torch.equal(oa, o)
        assert torch.equal(qa.grad, dq)
        assert torch.equal(ka.grad, dk)
        assert torch.equal(va.grad, dv)


def test_rejects_bad_tables():
    q, k, v, _dout, start, _scale = _inputs("small")
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, doc=start.long())
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, doc=start[:, :-1])
    with pytest.raises(ValueError):
        ops.flash_attention(q, k, v, doc=start.cpu())
    with pytest.raises(RuntimeError):
        ext().attn_fwd_doc(q, k, v, start.long(), 0.125)


# ---- 6. model ----
def test_llama_gpu_documents_are_isolated():
    from distributed_training_guide_amd.models import build_model

    torch.manual_seed(1)
    model = build_model("llama-debug", device=torch.device("cuda"),
                        dtype=torch.bfloat16)
    ids = torch.randint(0, 1024, (2, 128), device="cuda")
    nA = 50
    start = torch.zeros(2, 128, dtype=torch.int32, device="cuda")
    start[:, nA:] = nA
    out = model(input_ids=ids, labels=ids, doc_start=start)
    out.loss.backward()
    assert torch.isfinite(out.loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())

    ids2 = ids.clone()
    ids2[:, :nA] = (ids[:, :nA] + 1) % 1024
    with torch.no_grad():
        a = model(input_ids=ids, doc_start=start).logits
        b = model(input_ids=ids2, doc_start=start).logits
        leaky = model(input_ids=ids2).logits
    assert not torch.equal(a[:, :nA], b[:, :nA])
    assert torch.equal(a[:, nA:], b[:, nA:])
    assert not torch.equal(a[:, nA:], leaky[:, nA:])
