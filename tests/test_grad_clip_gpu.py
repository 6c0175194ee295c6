"""GPU tests of the fused global grad-norm clipping: grad_norm.hip
(grad_sq_sum / clip_grad_norm_) and the clipped AdamW kernel
(FusedAdamW(max_grad_norm=...)) against torch references."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from distributed_training_guide_amd import ops

# (262145,) spills one element into a second 262144-element chunk
SHAPES = [(3,), (333, 55), (1024,), (262144,), (262145,)]
DTYPES = {
    "bf16": [torch.bfloat16] * 5,
    "fp32": [torch.float32] * 5,
    "mixed": [torch.bfloat16, torch.float32, torch.bfloat16, torch.float32,
              torch.bfloat16],
}


def _rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _with_grad(g):
    """A parameter-like tensor whose .grad IS `g` (views keep their base)."""
    p = torch.zeros(g.shape, dtype=g.dtype, device=g.device,
                    requires_grad=True)
    p.grad = g
    return p


def _params(shapes, dtypes, seed=0):
    torch.manual_seed(seed)
    return [_with_grad(torch.randn(*s, device="cuda").to(dt))
            for s, dt in zip(shapes, dtypes)]


def _sq_ref(params):
    return sum(p.grad.double().pow(2).sum() for p in params)


# rtol 1e-4 on the squared sum: all terms are non-negative, so the relative
# error is <= (longest sequential fp32 add chain) * 2^-24; the chain is
# <= 1024 per thread plus the reduce stages -> ~6.6e-5.

@pytest.mark.parametrize("kind", ["bf16", "fp32", "mixed"])
def test_grad_sq_sum_matches_fp64(kind):
    params = _params(SHAPES, DTYPES[kind])
    params.append(torch.zeros(4, device="cuda", requires_grad=True))  # None
    out = ops.grad_sq_sum(params)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.is_cuda
    ref = _sq_ref(params[:-1])
    print(f"sq_sum {kind}: rel err {abs(out.item() - ref.item()) / ref.item():.3e}")
    torch.testing.assert_close(out.double(), ref, rtol=1e-4, atol=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grad_sq_sum_unaligned_base(dtype):
    torch.manual_seed(1)
    n = 18315
    buf = torch.randn(n + 8, device="cuda").to(dtype)
    g = buf[1:1 + n]  # element-aligned only: not 16 B aligned
    assert g.data_ptr() % 16 != 0
    p = _with_grad(g)
    assert p.grad.data_ptr() == g.data_ptr()
    out = ops.grad_sq_sum([p])
    torch.testing.assert_close(out.double(), _sq_ref([p]), rtol=1e-4, atol=0)


def test_grad_sq_sum_reproducible():
    params = _params(SHAPES, DTYPES["mixed"], seed=2)
    a = ops.grad_sq_sum(params).clone()
    b = ops.grad_sq_sum(params).clone()
    assert torch.equal(a, b)


def _bf16_bits(t):
    return t.view(torch.int16).to(torch.int32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_clip_grad_norm_matches_torch(dtype):
    shapes = [(3,), (333, 55), (1024,), (262145,)]
    params = _params(shapes, [dtype] * 4, seed=3)
    ref = [_with_grad(p.grad.float().clone()) for p in params]
    norm_ref = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    coef_ref = (1.0 / (norm_ref + 1e-6)).clamp(max=1.0)
    assert coef_ref.item() < 1.0  # clipping is active
    before = [p.grad.clone() for p in params]
    norm = ops.clip_grad_norm_(params, 1.0)
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.is_cuda
    torch.testing.assert_close(norm, norm_ref, rtol=1e-4, atol=0)
    for p, pr, g0 in zip(params, ref, before):
        if dtype == torch.float32:
            torch.testing.assert_close(p.grad, pr.grad, rtol=1e-4, atol=0)
        else:
            want = (g0.float() * coef_ref).bfloat16()
            ulps = (_bf16_bits(p.grad) - _bf16_bits(want)).abs().max().item()
            assert ulps <= 1, ulps


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_clip_grad_norm_inactive_leaves_grads(dtype):
    params = _params(SHAPES, [dtype] * 5, seed=4)
    before = [p.grad.clone() for p in params]
    ops.clip_grad_norm_(params, 1e30)  # coef is exactly 1
    for p, g0 in zip(params, before):
        assert torch.equal(p.grad, g0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_clip_grad_norm_unaligned_base(dtype):
    """The in-place scale peels the same scalar head as the norm and must
    not touch the elements around the view."""
    torch.manual_seed(5)
    n = 18315
    buf = torch.randn(n + 8, device="cuda").to(dtype)
    orig = buf.clone()
    p = _with_grad(buf[1:1 + n])
    norm = ops.clip_grad_norm_([p], 1.0)
    coef = (1.0 / (norm + 1e-6)).clamp(max=1.0)
    want = (orig[1:1 + n].float() * coef).to(dtype)
    if dtype == torch.float32:
        torch.testing.assert_close(buf[1:1 + n], want, rtol=1e-6, atol=0)
    else:
        ulps = (_bf16_bits(buf[1:1 + n].contiguous())
                - _bf16_bits(want)).abs().max().item()
        assert ulps <= 1, ulps
    assert torch.equal(buf[:1], orig[:1])
    assert torch.equal(buf[1 + n:], orig[1 + n:])


# ---------------- fused into FusedAdamW ----------------
# 1e-4 where the unclipped fp32 test uses 1e-5: the scale itself carries up
# to ~5e-5 relative error from the fp32 norm.

def test_fused_adamw_clipped_fp32():
    torch.manual_seed(1)
    p_hip = torch.randn(2048, 128, device="cuda", requires_grad=True)
    p_ref = p_hip.detach().clone().requires_grad_(True)
    opt_hip = ops.FusedAdamW([p_hip], lr=3e-3, weight_decay=0.05,
                             max_grad_norm=1.0)
    opt_ref = torch.optim.AdamW([p_ref], lr=3e-3, weight_decay=0.05)
    assert opt_hip.last_grad_norm is None
    for _ in range(3):
        g = torch.randn_like(p_ref)
        p_hip.grad = g.clone()
        p_ref.grad = g.clone()
        opt_hip.step()
        norm_ref = torch.nn.utils.clip_grad_norm_([p_ref], 1.0)
        opt_ref.step()
        assert torch.equal(p_hip.grad, g)  # grads are never rewritten
        torch.testing.assert_close(opt_hip.last_grad_norm, norm_ref,
                                   rtol=1e-4, atol=0)
    assert opt_hip.last_grad_norm.dim() == 0
    assert opt_hip.last_grad_norm.dtype == torch.float32
    err = _rel_err(p_hip, p_ref)
    print(f"clipped fp32 adamw rel err {err:.3e}")
    assert err < 1e-4


def test_fused_adamw_clipped_bf16():
    torch.manual_seed(0)
    shapes = [(1024,), (333, 55), (4096, 64)]
    params_hip = [torch.randn(*s, device="cuda", dtype=torch.bfloat16,
                              requires_grad=True) for s in shapes]
    params_ref = [p.detach().float().clone().requires_grad_(True)
                  for p in params_hip]
    opt_hip = ops.FusedAdamW(params_hip, lr=1e-2, weight_decay=0.1,
                             max_grad_norm=1.0)
    opt_ref = torch.optim.AdamW(params_ref, lr=1e-2, weight_decay=0.1)
    for step in range(5):
        for p, pr in zip(params_hip, params_ref):
            gb = torch.randn_like(pr).to(torch.bfloat16)
            p.grad = gb
            pr.grad = gb.float()
        keep = [p.grad.clone() for p in params_hip]
        opt_hip.step()
        norm_ref = torch.nn.utils.clip_grad_norm_(params_ref, 1.0)
        opt_ref.step()
        torch.testing.assert_close(opt_hip.last_grad_norm, norm_ref,
                                   rtol=1e-4, atol=0)
        for p, g0 in zip(params_hip, keep):
            assert torch.equal(p.grad, g0)
    for p, pr in zip(params_hip, params_ref):
        assert _rel_err(p, pr) < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fused_adamw_huge_max_norm_is_bit_identical(dtype):
    """max_grad_norm=1e30 runs the clipped kernel with coef exactly 1: the
    params and moments must equal the default optimizer's bit for bit."""
    torch.manual_seed(6)
    shapes = [(1024,), (333, 55), (4096, 64)]
    pa = [torch.randn(*s, device="cuda").to(dtype).requires_grad_(True)
          for s in shapes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa = ops.FusedAdamW(pa, lr=1e-2, weight_decay=0.1, max_grad_norm=1e30)
    ob = ops.FusedAdamW(pb, lr=1e-2, weight_decay=0.1)
    for _ in range(3):
        for x, y in zip(pa, pb):
            g = torch.randn_like(x)
            x.grad = g.clone()
            y.grad = g.clone()
        oa.step()
        ob.step()
    assert ob.last_grad_norm is None
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][k], ob.state[y][k]), k


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_grad_reported(bad):
    torch.manual_seed(7)
    params = [torch.randn(333, 55, device="cuda", requires_grad=True),
              torch.randn(1024, device="cuda", requires_grad=True)]
    opt = ops.FusedAdamW(params, lr=1e-3, max_grad_norm=1.0)
    for p in params:
        p.grad = torch.randn_like(p)
    params[0].grad[17, 3] = bad
    opt.step()
    norm = opt.last_grad_norm.item()
    assert math.isnan(norm) if math.isnan(bad) else norm == math.inf


def test_clipped_step_does_not_sync():
    torch.manual_seed(8)
    params = [torch.randn(333, 55, device="cuda", dtype=torch.bfloat16,
                          requires_grad=True),
              torch.randn(4096, 64, device="cuda", dtype=torch.bfloat16,
                          requires_grad=True)]
    opt = ops.FusedAdamW(params, lr=1e-3, max_grad_norm=1.0)
    grads = [torch.randn_like(p) for p in params]  # stable addresses
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()  # warm-up: builds and caches the descriptor tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert math.isfinite(opt.last_grad_norm.item())


def test_llama_debug_trains_with_clipping():
    from distributed_training_guide_amd.models import build_model

    torch.manual_seed(0)
    model = build_model("llama-debug", device="cuda", dtype=torch.bfloat16)
    opt = ops.FusedAdamW(model.parameters(), lr=1e-3, max_grad_norm=1.0)
    ids = torch.randint(0, 1024, (2, 128), device="cuda")
    losses, norms = [], []
    for _ in range(5):
        out = model(input_ids=ids, labels=ids)
        out.loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        losses.append(out.loss.item())
        norms.append(opt.last_grad_norm.item())
    assert all(math.isfinite(l) for l in losses)
    assert losses[-1] < losses[0]
    # the init norm measures 6.1-6.8 on this model: clipping is active
    assert all(math.isfinite(n) and n > 1.0 for n in norms), norms
