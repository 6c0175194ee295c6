"""Proof, without a GPU, of the checker and bounds in tests/utils_numerics.py.

1. The project's eager f32 paths (ops/reference.py, F.embedding, F.gelu,
   FusedAdamW._step_eager) pass every bound against the fp64 references on
   the GPU tests' own input recipes: the bounds are attainable by a correct
   f32 implementation and the inputs sit on no cancellation the `mag` terms
   fail to cover.  Sizes that exist only to trip a GPU grid-stride are
   shrunk.
2. Each kind of damage a subtly wrong kernel would produce is rejected.
3. The -inf cross-entropy recipe has a finite fp64 reference and
   F.cross_entropy agrees with it."""
import pytest
import torch
import torch.nn.functional as F

import utils_numerics as N
from distributed_training_guide_amd.ops import FusedAdamW
from distributed_training_guide_amd.ops import reference as R

CPU = "cpu"


# ---------------- the checker itself ----------------
def test_checker_nonfinite_rules():
    ref = torch.tensor([1.0, float("inf"), -float("inf"), 2.0],
                       dtype=torch.float64)
    N.assert_bf16_close(ref.bfloat16(), ref)
    N.assert_f32_close(ref.float(), ref, 1e-6, 0.0)
    for bad in ([1.0, -float("inf"), -float("inf"), 2.0],   # sign of inf
                [1.0, float("inf"), -float("inf"), float("nan")],
                [float("inf"), float("inf"), -float("inf"), 2.0],
                [1.0, 3e38, -float("inf"), 2.0]):           # finite for inf
        y = torch.tensor(bad)
        with pytest.raises(AssertionError):
            N.assert_bf16_close(y.bfloat16(), ref)
        with pytest.raises(AssertionError):
            N.assert_f32_close(y, ref, 1e-6, 0.0)


def test_checker_report_names_worst_element():
    ref = torch.linspace(1.0, 2.0, 24, dtype=torch.float64).view(2, 3, 4)
    y = ref.bfloat16()
    y[1, 2, 3] = 3.0
    y[0, 1, 1] = 1.5
    with pytest.raises(AssertionError) as e:
        N.assert_bf16_close(y, ref, what="probe")
    msg = str(e.value)
    assert "probe" in msg and "2 of 24" in msg and "(1, 2, 3)" in msg
    assert "bound" in msg and "3.0" in msg


def test_checker_bound_is_half_ulp_not_more():
    # 1 + 2^-8 is the midpoint of two bf16 neighbours: either is in bound,
    # the next one out is not
    ref = torch.full((4,), 1.0 + 2.0 ** -8, dtype=torch.float64)
    ok = torch.tensor([1.0, 1.0078125, 1.0, 1.0078125]).bfloat16()
    N.assert_bf16_close(ok, ref)
    with pytest.raises(AssertionError):
        N.assert_bf16_close(N.bump_bf16_ulps(ok, 1, 1), ref)


# ---------------- silu_mul ----------------
SILU_SHAPES = [(1, 8), (5, 520), (3, 1408), (70, 8)]  # (8200, 8) shrunk


def _silu_eager(gu, dy):
    g = gu.clone().requires_grad_(True)
    y = R.silu_mul_ref(g)
    y.backward(dy)
    I = gu.shape[-1] // 2
    return y.detach(), g.grad[..., :I], g.grad[..., I:]


@pytest.mark.parametrize("rows,I", SILU_SHAPES)
def test_silu_eager_passes(rows, I):
    gu, dy = N.silu_inputs(rows, I, CPU)
    y, dg, du = _silu_eager(gu, dy)
    N.assert_bf16_close(y, N.silu_mul_ref64(gu), what="silu y")
    rg, mg, ru = N.silu_mul_bwd_ref64(dy, gu)
    N.assert_bf16_close(dg.contiguous(), rg, mg, "silu dg")
    N.assert_bf16_close(du.contiguous(), ru, what="silu du")


def test_silu_damage_is_rejected():
    gu, dy = N.silu_inputs(5, 520, CPU)
    y, _, _ = _silu_eager(gu, dy)
    ref = N.silu_mul_ref64(gu)
    N.assert_bf16_close(y, ref)
    worst = tuple(int(i) for i in (ref.abs() == ref.abs().max()).nonzero()[0])
    with pytest.raises(AssertionError):       # one element, 2 bf16 ulps
        N.assert_bf16_close(N.bump_bf16_ulps(y, worst, 2), ref)
    swapped = y.clone()
    swapped[[1, 3]] = y[[3, 1]]
    with pytest.raises(AssertionError):       # two rows exchanged
        N.assert_bf16_close(swapped, ref)
    shifted = y.clone()
    shifted[2, 256:264] = y[2, 264:272]
    with pytest.raises(AssertionError):       # one 8-lane group, 8 columns
        N.assert_bf16_close(shifted, ref)
    I = 520
    f32 = F.silu(gu[..., :I].float()) * gu[..., I:].float()
    with pytest.raises(AssertionError):       # truncation, not rounding
        N.assert_bf16_close(N.truncate_to_bf16(f32), ref)


# ---------------- rope ----------------
ROPE_CASES = [
    # (B, S, H, D, theta, positions)
    (1, 5, 2, 8, 1e4, False),
    (2, 17, 3, 64, 5e5, False),
    (2, 17, 3, 128, 1e4, True),
    (2, 130, 5, 128, 5e5, False),   # (2,130,33,128) shrunk in H
    (2, 33, 4, 64, 1e4, True),
]


@pytest.mark.parametrize("B,S,H,D,theta,use_pos", ROPE_CASES)
def test_rope_eager_passes(B, S, H, D, theta, use_pos):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, S, H, D, generator=g).bfloat16()
    max_pos = S + 40
    cos, sin = R.rope_tables(D, max_pos, theta)
    pos = N.rope_positions(S, max_pos, CPU) if use_pos else None
    if use_pos:
        assert int(pos.max()) == max_pos - 1 > S
        assert (pos[1:] < pos[:-1]).any() and pos.unique().numel() < S
    for backward in (False, True):
        y = R.rope_ref(x, cos, sin, pos, backward=backward)
        ref, mag = N.rope_ref64(x, cos, sin, pos, backward)
        N.assert_bf16_close(y, ref, mag, f"rope bwd={backward}")
    # rotation is orthogonal: backward of forward returns the input
    y = R.rope_ref(x, cos, sin, pos)
    back = R.rope_ref(y, cos, sin, pos, backward=True)
    ref, mag = N.rope_ref64(y, cos, sin, pos, True)
    N.assert_bf16_close(back, ref, mag, "rope backward(forward)")
    N.assert_bf16_close(back, x.double(), N.ROPE_ROUND_TRIP * mag,
                        "rope round trip")


@pytest.mark.parametrize("use_pos", [False, True])
@pytest.mark.parametrize("B,S,Hq,Hkv,D", [
    (1, 3, 1, 1, 16), (2, 17, 4, 1, 32), (2, 33, 8, 2, 64), (2, 33, 8, 2, 128),
    (2, 70, 4, 2, 128),   # (2,1400,32,8,128) shrunk
])
def test_qkv_rope_eager_passes(B, S, Hq, Hkv, D, use_pos):
    from distributed_training_guide_amd import ops
    from distributed_training_guide_amd.ops.rope import get_rope_tables

    g = torch.Generator().manual_seed(21)
    W = (Hq + 2 * Hkv) * D
    qkv = torch.randn(B, S, W, generator=g).bfloat16().requires_grad_(True)
    max_pos = S + 40
    pos = N.rope_positions(S, max_pos, CPU) if use_pos else None
    cos, sin = get_rope_tables(D, max_pos, 1e4, qkv.device)
    q, k, v = ops.qkv_rope(qkv, Hq, Hkv, D, theta=1e4, positions=pos,
                           max_pos=max_pos)
    x = qkv.detach()
    q_in = x[..., :Hq * D].reshape(B, S, Hq, D)
    k_in = x[..., Hq * D:(Hq + Hkv) * D].reshape(B, S, Hkv, D)
    assert torch.equal(v, x[..., (Hq + Hkv) * D:].reshape(B, S, Hkv, D))
    for name, got, src in (("q", q, q_in), ("k", k, k_in)):
        ref, mag = N.rope_ref64(src, cos, sin, pos)
        N.assert_bf16_close(got.detach(), ref, mag, "eager qkv_rope " + name)
    dq = torch.randn(B, S, Hq, D, generator=g).bfloat16()
    dk = torch.randn(B, S, Hkv, D, generator=g).bfloat16()
    dv = torch.randn(B, S, Hkv, D, generator=g).bfloat16()
    torch.autograd.backward([q, k, v], [dq, dk, dv])
    rq, mq = N.rope_ref64(dq, cos, sin, pos, True)
    rk, mk = N.rope_ref64(dk, cos, sin, pos, True)
    ref = torch.cat([rq.reshape(B, S, -1), rk.reshape(B, S, -1),
                     dv.double().reshape(B, S, -1)], dim=-1)
    mag = torch.cat([mq.reshape(B, S, -1), mk.reshape(B, S, -1),
                     dv.double().abs().reshape(B, S, -1)], dim=-1)
    N.assert_bf16_close(qkv.grad, ref, mag, "eager qkv_rope dqkv")


def test_rope_half_swap_is_rejected():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, 3, 64, generator=g).bfloat16()
    cos, sin = R.rope_tables(64, 64, 1e4)
    y = R.rope_ref(x, cos, sin)
    ref, mag = N.rope_ref64(x, cos, sin)
    N.assert_bf16_close(y, ref, mag)
    bad = y.clone()
    bad[1, 4, 2, :32] = y[1, 4, 2, 32:]
    bad[1, 4, 2, 32:] = y[1, 4, 2, :32]
    with pytest.raises(AssertionError):
        N.assert_bf16_close(bad, ref, mag)


# ---------------- cross entropy ----------------
CE_SHAPES = [(1, 2, 8), (2, 9, 2056), (3, 700, 64), (2, 64, 512)]


def _ce_eager_rows(logits, labels):
    B, S, V = logits.shape
    x = logits[:, :-1].float().reshape(-1, V)
    tgt = labels[:, 1:].reshape(-1)
    loss = F.cross_entropy(x, tgt, ignore_index=N.IGNORE_INDEX,
                           reduction="none")
    return loss, torch.logsumexp(x, dim=-1)


@pytest.mark.parametrize("recipe", N.CE_RECIPES)
@pytest.mark.parametrize("B,S,V", CE_SHAPES)
def test_ce_eager_passes(B, S, V, recipe):
    logits, labels = N.ce_inputs(B, S, V, recipe, CPU)
    ref = N.ce_ref64(logits, labels)
    assert ref["n_valid"] >= 1
    assert torch.isfinite(ref["loss"]).all()
    assert torch.isfinite(ref["lse_all"]).all()
    mag = N.ce_row_mag(ref)
    loss, lse = _ce_eager_rows(logits, labels)
    N.assert_f32_close(loss, ref["loss"], N.CE_ROW_RTOL, N.CE_ROW_ATOL, mag,
                       "eager loss rows")
    N.assert_f32_close(lse, ref["lse_all"], N.CE_ROW_RTOL, N.CE_ROW_ATOL,
                       mag, "eager lse")
    # the kernel's own algorithm (online max / rescaled sum per thread) in
    # CPU f32 stays inside the derived bound too
    N.assert_f32_close(N.ce_online_f32(logits), ref["lse_all"],
                       N.CE_ROW_RTOL, N.CE_ROW_ATOL, mag, "online-f32 lse")
    # gradients, plain mean and with an upstream factor
    for up in (1.0, 3.5):
        x = logits.clone().requires_grad_(True)
        (R.cross_entropy_ref(x, labels) * up).backward()
        d, m = N.ce_dlogits_ref64(logits, ref, up / ref["n_valid"])
        N.assert_bf16_close(x.grad, d, m, f"eager dlogits x{up}")
        assert torch.equal(x.grad[:, -1], torch.zeros_like(x.grad[:, -1]))


def test_ce_neginf_recipe_is_finite_and_matches_torch():
    for B, S, V in CE_SHAPES:
        logits, labels = N.ce_inputs(B, S, V, "neginf", CPU)
        cols = N.ce_neginf_columns(V)
        assert 0 in cols and torch.isinf(logits[..., cols]).all()
        if V >= 32:
            assert set(range(16)) <= set(cols)
        tgt = labels[labels != N.IGNORE_INDEX]
        assert torch.isfinite(logits[0, 0, tgt]).all()  # labels on finite cols
        ref = N.ce_ref64(logits, labels)
        assert torch.isfinite(ref["loss"]).all()
        mean = R.cross_entropy_ref(logits, labels)
        assert torch.isfinite(mean)
        want = ref["loss"].sum() / ref["n_valid"]
        assert abs(mean.item() - want.item()) <= 2.0 ** -21 * abs(
            want.item()) * 4 + N.CE_ROW_ATOL


@pytest.mark.parametrize("B,S,V,tp,owners", [
    (2, 9, 96, 3, 3), (2, 9, 96, 3, 2), (2, 9, 4160, 2, 2), (3, 700, 64, 2, 2),
])
def test_ce_sharded_combine_eager_passes(B, S, V, tp, owners):
    """The shard-wise (max, sum, gathered) combine in eager f32 meets the
    bounds the sharded GPU test applies."""
    g = torch.Generator().manual_seed(31)
    full = torch.randn(B, S, V, generator=g).bfloat16()
    labels = N.ce_sharded_labels(B, S, V, tp, owners)
    Vl = V // tp
    tgt = labels[:, 1:].reshape(-1)
    valid = tgt != N.IGNORE_INDEX
    assert int(tgt.max()) == owners * Vl - 1 and (~valid).any()
    for r in range(1, owners):
        assert (tgt == r * Vl - 1).any() and (tgt == r * Vl).any()
    ref = N.ce_ref64(full, labels)
    mx, sm = [], []
    for r in range(tp):
        shard = full[..., r * Vl:(r + 1) * Vl]
        rows = shard[:, :-1].float().reshape(-1, Vl)
        m = rows.amax(-1)
        s = torch.exp(rows - m.unsqueeze(-1)).sum(-1)
        N.assert_f32_close(s, N.ce_shard_sum_ref64(shard), N.CE_SUM_RTOL, 0.0,
                           what=f"eager sumout {r}")
        mx.append(m), sm.append(s)
    gmax = torch.stack(mx).amax(0)
    lse = gmax + torch.log(sum(s * torch.exp(m - gmax)
                               for s, m in zip(sm, mx)))
    N.assert_f32_close(lse, ref["lse_all"], N.CE_ROW_RTOL, N.CE_ROW_ATOL,
                       N.ce_row_mag(ref), "eager combined lse")


def test_ce_shifted_onehot_is_rejected():
    logits, labels = N.ce_inputs(2, 64, 512, "normal", CPU)
    ref = N.ce_ref64(logits, labels)
    scale = 1.0 / ref["n_valid"]
    d, m = N.ce_dlogits_ref64(logits, ref, scale)
    N.assert_bf16_close(d.bfloat16(), d, m)
    wrong, _ = N.ce_dlogits_ref64(logits, ref, scale, label_shift=1)
    with pytest.raises(AssertionError):
        N.assert_bf16_close(wrong.bfloat16(), d, m)


# ---------------- gelu ----------------
@pytest.mark.parametrize("numel", [8, 3 * 104, 4096 + 8])  # 8,388,616 shrunk
def test_gelu_eager_passes(numel):
    x, dy = N.gelu_inputs(numel, CPU)
    xg = x.clone().requires_grad_(True)
    y = F.gelu(xg, approximate="tanh")
    y.backward(dy)
    ref, mag = N.gelu_ref64(x)
    N.assert_bf16_close(y.detach(), ref, mag, "gelu y")
    rd, md = N.gelu_bwd_ref64(dy, x)
    N.assert_bf16_close(xg.grad, rd, md, "gelu dx")


def test_gelu_truncation_is_rejected():
    x, _ = N.gelu_inputs(4096, CPU)
    ref, mag = N.gelu_ref64(x)
    y32 = F.gelu(x.float(), approximate="tanh")
    N.assert_bf16_close(y32.bfloat16(), ref, mag)
    with pytest.raises(AssertionError):
        N.assert_bf16_close(N.truncate_to_bf16(y32), ref, mag)


# ---------------- AdamW ----------------
PAIRINGS = [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
            (torch.float32, torch.float32), (torch.float32, torch.bfloat16)]


def _adamw_one_step(hyper, k, p_dtype, g_dtype, sizes, device, f32_hyper):
    return N.adamw_one_step(FusedAdamW, hyper, k, p_dtype, g_dtype, sizes,
                            device, f32_hyper)


@pytest.mark.parametrize("k", [1, 1000])
@pytest.mark.parametrize("hyper", N.ADAMW_HYPER, ids=["lr1e-2", "defaults"])
@pytest.mark.parametrize("p_dtype,g_dtype", PAIRINGS)
def test_adamw_eager_passes(p_dtype, g_dtype, hyper, k):
    # all sizes: among 262155 elements some have beta1*m and (1-beta1)*g
    # cancelling, which is where the bound on p has to hold too
    sizes = N.ADAMW_SIZES
    for n, (p, m, v, ref) in zip(sizes, _adamw_one_step(
            hyper, k, p_dtype, g_dtype, sizes, CPU, f32_hyper=True)):
        N.assert_adamw_close(p, m, v, ref, f"n={n}")


def test_adamw_stale_second_moment_is_rejected():
    hyper, k = N.ADAMW_HYPER[1], 1000
    (p, m, v, ref), = _adamw_one_step(hyper, k, torch.float32, torch.float32,
                                      (18315,), CPU, f32_hyper=True)
    N.assert_adamw_close(p, m, v, ref)
    _, _, _, v0 = N.adamw_state(18315, torch.float32, torch.float32, CPU)
    with pytest.raises(AssertionError, match="exp_avg_sq"):
        N.assert_adamw_close(p, m, v0, ref)
    # and the parameter such a step would produce is rejected as well
    h = N.adamw_f32_hyper(hyper)
    p0, g0, m0, _ = N.adamw_state(18315, torch.float32, torch.float32, CPU)
    bc1 = 1.0 - h["betas"][0] ** k
    bc2 = 1.0 - h["betas"][1] ** k
    stale = p0.double() * (1 - h["lr"] * h["weight_decay"]) - h["lr"] * (
        ref["m"] / bc1) / (torch.sqrt(v0.double() / bc2) + h["eps"])
    with pytest.raises(AssertionError):
        N.assert_adamw_close(stale.float(), m, v, ref)


# ---------------- embedding ----------------
@pytest.mark.parametrize("V,H,ids_shape,all_equal", [
    (64, 8, (10,), False), (40, 100, (4, 64), False), (3, 50, (7,), False),
    (1, 3, (5,), False),
    (16, 8, (33000,), False), (16, 8, (33000,), True),
])
def test_embedding_recipe_is_exact(V, H, ids_shape, all_equal):
    table, ids, dy = N.embedding_inputs(V, H, ids_shape, CPU,
                                        all_equal=all_equal)
    assert torch.equal(F.embedding(ids, table), table[ids])
    # f32 accumulation of this dy is exact in any order, so the eager f32
    # scatter rounded once equals the fp64 one
    w = table.float().requires_grad_(True)
    F.embedding(ids, w).backward(dy.float())
    ref = N.embedding_bwd_ref(dy, ids, V)
    assert torch.equal(w.grad.bfloat16(), ref)
    hit = torch.zeros(V, dtype=torch.bool)
    hit[ids.reshape(-1)] = True
    assert torch.equal(ref[~hit], torch.zeros_like(ref[~hit]))
    # one lost update is visible
    lost = torch.zeros(V, H, dtype=torch.float64)
    flat_ids, flat_dy = ids.reshape(-1), dy.reshape(-1, H).double()
    lost.index_add_(0, flat_ids[1:], flat_dy[1:])
    if (flat_dy[0] != 0).any() and ids.numel() < 1000:
        assert not torch.equal(lost.bfloat16(), ref)
