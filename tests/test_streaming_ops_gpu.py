"""Per-element fp64 checks of the streaming HIP kernels: silu_mul, rope,
qkv_rope, cross entropy, embedding, tanh-GELU and AdamW.

Each case compares the kernel with a plain fp64 reference of the same
operation on the same bf16 / f32 inputs, element by element, under the
bounds derived in tests/utils_numerics.py (shown attainable by the eager f32
paths in tests/test_numerics_helper_cpu.py).  Shapes are the smallest that
reach the branch named beside them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import utils_numerics as N
from distributed_training_guide_amd import ops
from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops.embedding import _EmbeddingFn
from distributed_training_guide_amd.ops.rope import get_rope_tables

DEV = "cuda"
IGN = N.IGNORE_INDEX


# ---------------- silu_mul ----------------
@pytest.mark.parametrize("rows,I", [
    (1, 8),      # one wave, one lane
    (5, 520),    # second lane-loop pass (i = 512) holds lane 0 only
    (3, 1408),   # the Llama-debug width: two full passes and a partial one
    (8200, 8),   # > 2048 blocks * 4 waves: rows 8192.. from the grid-stride
])
def test_silu_mul(rows, I):
    gu, dy = N.silu_inputs(rows, I, DEV)
    y = ext().silu_mul_fwd(gu)
    N.assert_bf16_close(y, N.silu_mul_ref64(gu), what="silu_mul y")
    dgu = ext().silu_mul_bwd(dy, gu)
    rg, mg, ru = N.silu_mul_bwd_ref64(dy, gu)
    N.assert_bf16_close(dgu[:, :I].contiguous(), rg, mg, "silu_mul dg")
    N.assert_bf16_close(dgu[:, I:].contiguous(), ru, what="silu_mul du")


def test_silu_mul_module_3d():
    gu, dy = N.silu_inputs(6, 520, DEV)
    gu3 = gu.view(2, 3, 1040).clone().requires_grad_(True)
    y = ops.silu_mul(gu3)
    assert y.shape == (2, 3, 520)
    y.backward(dy.view(2, 3, 520))
    N.assert_bf16_close(y.detach().view(6, 520), N.silu_mul_ref64(gu),
                        what="ops.silu_mul y")
    rg, mg, ru = N.silu_mul_bwd_ref64(dy, gu)
    g = gu3.grad.view(6, 1040)
    N.assert_bf16_close(g[:, :520].contiguous(), rg, mg, "ops.silu_mul dg")
    N.assert_bf16_close(g[:, 520:].contiguous(), ru, what="ops.silu_mul du")


# ---------------- rope ----------------
def _randn_bf16(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).bfloat16().to(DEV)


def _check_rope(x, cos, sin, pos):
    for backward in (False, True):
        y = ext().rope(x, cos, sin, pos, backward)
        ref, mag = N.rope_ref64(x, cos, sin, pos, backward)
        N.assert_bf16_close(y, ref, mag, f"rope backward={backward}")
    # rotation is orthogonal: backward of forward returns the input
    y = ext().rope(x, cos, sin, pos, False)
    back = ext().rope(y, cos, sin, pos, True)
    ref, mag = N.rope_ref64(y, cos, sin, pos, True)
    N.assert_bf16_close(back, ref, mag, "rope backward(forward)")
    N.assert_bf16_close(back, x.double(), N.ROPE_ROUND_TRIP * mag,
                        "rope round trip")


@pytest.mark.parametrize("theta", [1e4, 5e5])
@pytest.mark.parametrize("shape", [
    (2, 17, 3, 8),       # D/2 = 4: sixteen rows per wave
    (2, 17, 3, 64),
    (2, 17, 3, 128),     # D/2 = 64: one row per wave
    (2, 130, 33, 128),   # 549120 pairs > 2048*256: grid-stride, B > 1
])
def test_rope(shape, theta):
    B, S, H, D = shape
    x = _randn_bf16(shape, 11)
    cos, sin = get_rope_tables(D, S, theta, x.device)
    _check_rope(x, cos, sin, None)


@pytest.mark.parametrize("D", [8, 64, 128])
def test_rope_positions(D):
    """Non-monotone positions with repeats and an offset past S, B = 2:
    every batch row must look its position up by s, not by b*S + s."""
    B, S, H = 2, 33, 5
    max_pos = S + 40
    pos = N.rope_positions(S, max_pos, DEV)
    x = _randn_bf16((B, S, H, D), 12)
    cos, sin = get_rope_tables(D, max_pos, 1e4, x.device)
    _check_rope(x, cos, sin, pos)
    # and through the public op with autograd
    xg = x.clone().requires_grad_(True)
    y = ops.rope(xg, theta=1e4, positions=pos, max_pos=max_pos)
    dy = _randn_bf16((B, S, H, D), 13)
    y.backward(dy)
    ref, mag = N.rope_ref64(x, cos, sin, pos, False)
    N.assert_bf16_close(y.detach(), ref, mag, "ops.rope y")
    ref, mag = N.rope_ref64(dy, cos, sin, pos, True)
    N.assert_bf16_close(xg.grad, ref, mag, "ops.rope dx")


# ---------------- fused qkv split + rope ----------------
@pytest.mark.parametrize("use_pos", [False, True])
@pytest.mark.parametrize("B,S,Hq,Hkv,D", [
    (1, 3, 1, 1, 16),        # one 8-pair block per head row
    (2, 17, 4, 1, 32),
    (2, 33, 8, 2, 64),
    (2, 33, 8, 2, 128),
    (2, 1400, 32, 8, 128),   # 1,075,200 items > 4096*256: grid-stride
])
def test_qkv_rope(B, S, Hq, Hkv, D, use_pos):
    """q, k and dqkv against fp64 on the project's table, independently of
    the rope kernel; v is a bit-exact copy."""
    W = (Hq + 2 * Hkv) * D
    qkv = _randn_bf16((B, S, W), 21)
    max_pos = S + 40
    pos = N.rope_positions(S, max_pos, DEV) if use_pos else None
    cos, sin = get_rope_tables(D, max_pos, 1e4, qkv.device)
    q, k, v = ext().qkv_rope_fwd(qkv, cos, sin, pos, Hq, Hkv, D)
    q_in = qkv[..., :Hq * D].reshape(B, S, Hq, D)
    k_in = qkv[..., Hq * D:(Hq + Hkv) * D].reshape(B, S, Hkv, D)
    v_in = qkv[..., (Hq + Hkv) * D:].reshape(B, S, Hkv, D)
    assert torch.equal(v, v_in)
    ref, mag = N.rope_ref64(q_in, cos, sin, pos)
    N.assert_bf16_close(q, ref, mag, "qkv_rope q")
    ref, mag = N.rope_ref64(k_in, cos, sin, pos)
    N.assert_bf16_close(k, ref, mag, "qkv_rope k")
    del ref, mag

    dq = _randn_bf16((B, S, Hq, D), 22)
    dk = _randn_bf16((B, S, Hkv, D), 23)
    dv = _randn_bf16((B, S, Hkv, D), 24)
    dqkv = ext().qkv_rope_bwd(dq, dk, dv, cos, sin, pos)
    assert dqkv.shape == (B, S, W)
    rq, mq = N.rope_ref64(dq, cos, sin, pos, True)
    rk, mk = N.rope_ref64(dk, cos, sin, pos, True)
    ref = torch.cat([rq.reshape(B, S, -1), rk.reshape(B, S, -1),
                     dv.double().reshape(B, S, -1)], dim=-1)
    mag = torch.cat([mq.reshape(B, S, -1), mk.reshape(B, S, -1),
                     dv.double().abs().reshape(B, S, -1)], dim=-1)
    N.assert_bf16_close(dqkv, ref, mag, "qkv_rope dqkv")
    assert torch.equal(dqkv[..., (Hq + Hkv) * D:],
                       dv.reshape(B, S, Hkv * D))


# ---------------- cross entropy, unsharded ----------------
def check_ce_rows(C, logits, labels, scale_up=1.0):
    """Per-row loss / lse and dlogits of the extension module `C` against
    fp64.  Bounds: rows within 2^-21 * (|lse| + |x_label|) + 2e-5 (__expf's
    argument scaling at |x - max| <~ 20 is 20 * 2^-24, add chains are at
    most 16 long at these V, __logf a few ulps; the CPU f32 emulation of
    the same online algorithm stays inside it on every case here, see
    test_numerics_helper_cpu.py::test_ce_eager_passes)."""
    B, S, V = logits.shape
    ref = N.ce_ref64(logits, labels)
    loss, lse = C.ce_fwd(logits, labels, S - 1, IGN)
    mag = N.ce_row_mag(ref)
    N.assert_f32_close(lse, ref["lse"], N.CE_ROW_RTOL, N.CE_ROW_ATOL, mag,
                       "ce lse rows")
    N.assert_f32_close(loss, ref["loss"], N.CE_ROW_RTOL, N.CE_ROW_ATOL, mag,
                       "ce loss rows")
    scale = scale_up / max(ref["n_valid"], 1)
    d = C.ce_bwd(logits, labels, lse, scale, S - 1, 0, IGN, False)
    rd, md = N.ce_dlogits_ref64(logits, ref, scale)
    N.assert_bf16_close(d, rd, md, "ce dlogits")
    assert torch.equal(d[:, -1], torch.zeros_like(d[:, -1]))
    return ref


CE_SHAPES = [
    (1, 2, 8),       # one loss row, one lane
    (2, 9, 2056),    # second column pass (i = 2048) holds one thread
    (3, 700, 64),    # 2097 loss rows > 2048 blocks: the row grid-stride
    (2, 64, 512),
]


@pytest.mark.parametrize("recipe", N.CE_RECIPES)
@pytest.mark.parametrize("B,S,V", CE_SHAPES)
def test_ce_rows_and_autograd(B, S, V, recipe):
    logits, labels = N.ce_inputs(B, S, V, recipe, DEV)
    ref = check_ce_rows(ext(), logits, labels)
    # the public op: mean over valid rows, and autograd through scale_ptr
    # with a non-unit upstream gradient
    want = ref["loss"].sum() / ref["n_valid"]
    mean_mag = (N.ce_row_mag(ref).sum() / ref["n_valid"]).reshape(())
    for up in (1.0, 3.5):
        x = logits.clone().requires_grad_(True)
        loss = ops.causal_lm_loss(x, labels)
        # every row is within the row bound, hence so is their mean; the
        # f32 sum of the n non-negative rows errs by at most n * 2^-24 of
        # their total (any order of adds), which is the second rtol term
        n = ref["n_valid"]
        N.assert_f32_close(
            loss.detach().reshape(()), want.reshape(()),
            N.CE_ROW_RTOL + 2.0 ** -24 * n, N.CE_ROW_ATOL, mean_mag,
            "causal_lm_loss")
        (loss * up).backward()
        rd, md = N.ce_dlogits_ref64(logits, ref, up / n)
        N.assert_bf16_close(x.grad, rd, md, f"causal_lm_loss grad x{up}")
        assert torch.equal(x.grad[:, -1], torch.zeros_like(x.grad[:, -1]))


@pytest.mark.parametrize("B,S,V", CE_SHAPES)
def test_ce_all_ignored(B, S, V):
    logits, _ = N.ce_inputs(B, S, V, "normal", DEV)
    labels = torch.full((B, S), IGN, dtype=torch.int64, device=DEV)
    loss_rows, lse = ext().ce_fwd(logits, labels, S - 1, IGN)
    assert torch.equal(loss_rows, torch.zeros_like(loss_rows))
    x = logits.clone().requires_grad_(True)
    loss = ops.causal_lm_loss(x, labels)
    assert loss.item() == 0.0
    (loss * 3.5).backward()
    assert torch.isfinite(x.grad).all()
    assert torch.equal(x.grad, torch.zeros_like(x.grad))


# ---------------- embedding ----------------
@pytest.mark.parametrize("V,H,ids_shape,all_equal", [
    (64, 8, (10,), False),          # vector gather, 4-wide scatter
    (40, 100, (4, 64), False),      # gather scalar path, scatter 4-wide path
    (3, 50, (7,), False),           # both scalar paths; V*H = 150: tail of 2
    (1, 3, (5,), False),            # V*H = 3: the convert pass is all tail
    (1024, 520, (8, 512), False),   # second lane-loop pass, rows never hit
    (16, 8, (33000,), False),       # > 32768 ids: grid-stride, ~2000 hits/row
    (16, 8, (33000,), True),        # all 33000 ids equal: one row takes all
])
def test_embedding_gather_scatter(V, H, ids_shape, all_equal):
    table, ids, dy = N.embedding_inputs(V, H, ids_shape, DEV,
                                        all_equal=all_equal)
    out = ext().embedding_fwd(table, ids)
    assert out.shape == (*ids_shape, H)
    assert torch.equal(out, table[ids])
    # every f32 partial sum of this dy is exact in any order, so the fp64
    # sum rounded once to bf16 is the only correct answer: a lost or
    # doubled atomic changes it
    dtable = ext().embedding_bwd(dy, ids, V)
    ref = N.embedding_bwd_ref(dy, ids, V)
    assert dtable.shape == (V, H)
    bad = (dtable != ref).nonzero()
    assert torch.equal(dtable, ref), (
        f"{bad.shape[0]} wrong elements, first at {bad[0].tolist()}: "
        f"{dtable[tuple(bad[0])].item()} vs {ref[tuple(bad[0])].item()}")
    hit = torch.zeros(V, dtype=torch.bool, device=DEV)
    hit[ids.reshape(-1)] = True
    if not all_equal and V == 1024:
        assert (~hit).any()
    assert torch.equal(dtable[~hit], torch.zeros_like(dtable[~hit]))


def test_embedding_autograd_matches_kernels():
    """The autograd wrapper ops.Embedding uses on the GPU (called directly:
    the module itself routes to torch under the determinism recipe, a
    process-wide switch other tests flip)."""
    table, ids, dy = N.embedding_inputs(40, 100, (4, 64), DEV)
    w = table.clone().requires_grad_(True)
    out = _EmbeddingFn.apply(ids, w)
    out.backward(dy)
    assert torch.equal(out, table[ids])
    assert torch.equal(w.grad, N.embedding_bwd_ref(dy, ids, 40))


# ---------------- gelu ----------------
@pytest.mark.parametrize("numel", [
    8,              # one vector
    3 * 104,        # 39 vectors in one block
    8_388_616,      # one vector past 4096*256*8: the grid-stride
])
def test_gelu(numel):
    x, dy = N.gelu_inputs(numel, DEV)
    y = ext().gelu_fwd(x)
    ref, mag = N.gelu_ref64(x)
    N.assert_bf16_close(y, ref, mag, "gelu y")
    del ref, mag
    dx = ext().gelu_bwd(dy, x)
    ref, mag = N.gelu_bwd_ref64(dy, x)
    N.assert_bf16_close(dx, ref, mag, "gelu dx")


# ---------------- AdamW ----------------
PAIRINGS = [
    (torch.bfloat16, torch.bfloat16),
    (torch.bfloat16, torch.float32),   # FSDP reduce_dtype=fp32
    (torch.float32, torch.float32),
    (torch.float32, torch.bfloat16),
]


@pytest.mark.parametrize("k", [1, 1000])
@pytest.mark.parametrize("hyper", N.ADAMW_HYPER, ids=["lr1e-2", "defaults"])
@pytest.mark.parametrize("p_dtype,g_dtype", PAIRINGS)
def test_adamw_one_step(p_dtype, g_dtype, hyper, k):
    """p, exp_avg and exp_avg_sq after step k from a known state.  Sizes:
    scalar tail only (1, 7), one vector (8), vector + tail (9), an odd
    mid size, exactly one chunk, and a second chunk holding one vector and
    a tail of 3 (262155)."""
    res = N.adamw_one_step(ops.FusedAdamW, hyper, k, p_dtype, g_dtype,
                           N.ADAMW_SIZES, DEV)
    for n, (p, m, v, ref) in zip(N.ADAMW_SIZES, res):
        N.assert_adamw_close(p, m, v, ref, f"adamw n={n}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_adamw_chunk_grid_stride(dtype):
    """16400 three-element parameters: more chunks than the 16384-block
    grid, so blocks 0..15 take a second chunk.  The parameters are views of
    flat buffers at a 16-byte pitch; the slots between them must not move."""
    n_par, pitch = 16400, 8
    hyper, k = N.ADAMW_HYPER[0], 1000
    total = n_par * pitch
    p0, g0, m0, v0 = N.adamw_state(total, dtype, dtype, DEV)
    pf, mf, vf = p0.clone(), m0.clone(), v0.clone()
    params = []
    for i in range(n_par):
        p = torch.nn.Parameter(pf[i * pitch:i * pitch + 3])
        p.grad = g0[i * pitch:i * pitch + 3]
        params.append(p)
    opt = ops.FusedAdamW(params, **hyper)
    for i, p in enumerate(params):
        opt.state[p]["exp_avg"] = mf[i * pitch:i * pitch + 3]
        opt.state[p]["exp_avg_sq"] = vf[i * pitch:i * pitch + 3]
    opt.param_groups[0]["step"] = k - 1
    opt.step()
    ref = N.adamw_ref64(p0, g0, m0, v0, hyper, k)
    used = (torch.arange(total, device=DEV) % pitch) < 3
    for name, start in (("p", p0), ("m", m0), ("v", v0)):
        ref[name] = torch.where(used, ref[name], start.double())
    ref["delta_mag"] = torch.where(used, ref["delta_mag"],
                                   torch.zeros_like(ref["delta_mag"]))
    N.assert_adamw_close(pf, mf, vf, ref, "adamw 16400 x 3")
    for got, start in ((pf, p0), (mf, m0), (vf, v0)):
        assert torch.equal(got[~used], start[~used])


# ---------------- input checks of the bindings ----------------
def test_bindings_reject_bad_inputs():
    """Every call below must raise before a kernel is launched."""
    C = ext()
    bf = dict(device=DEV, dtype=torch.bfloat16)
    f32 = dict(device=DEV, dtype=torch.float32)
    logits = torch.zeros(2, 4, 16, **bf)
    labels = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    lse = torch.zeros(6, **f32)
    x = torch.zeros(1, 4, 2, 16, **bf)
    cos, sin = torch.zeros(8, 8, **f32), torch.zeros(8, 8, **f32)
    pos = torch.zeros(4, dtype=torch.int32, device=DEV)
    qkv = torch.zeros(1, 4, 4 * 16, **bf)
    dq, dk = torch.zeros(1, 4, 2, 16, **bf), torch.zeros(1, 4, 1, 16, **bf)
    gu, dy = torch.zeros(3, 32, **bf), torch.zeros(3, 16, **bf)
    table = torch.zeros(5, 8, **bf)
    ids = torch.zeros(3, dtype=torch.int64, device=DEV)

    def fwd_sh(lg=logits, lb=labels, s_out=3):
        return C.ce_fwd_sharded(lg, lb, s_out, 0, IGN)

    def bwd(lg=logits, lb=labels, ls=lse, s_out=3):
        return C.ce_bwd(lg, lb, ls, 1.0, s_out, 0, IGN, False)

    bad = [
        # ce_fwd_sharded
        lambda: fwd_sh(lg=logits[0]),                         # not 3-D
        lambda: fwd_sh(lb=labels.int()),                      # not int64
        lambda: fwd_sh(lb=labels.t()),                        # not [B,S]
        lambda: fwd_sh(lb=torch.zeros(2, 8, dtype=torch.int64,
                                      device=DEV)[:, ::2]),   # not contiguous
        lambda: fwd_sh(lb=labels.cpu()),                      # other device
        lambda: fwd_sh(s_out=0),
        lambda: fwd_sh(s_out=5),                              # S_out > S
        lambda: fwd_sh(lg=torch.zeros(2, 4, 12, **bf)),       # V % 8
        # ce_bwd
        lambda: bwd(lg=logits[0]),
        lambda: bwd(lb=labels.int()),
        lambda: bwd(lb=labels.t()),
        lambda: bwd(lb=labels.cpu()),
        lambda: bwd(s_out=0),
        lambda: bwd(s_out=5),
        lambda: bwd(lg=torch.zeros(2, 4, 12, **bf)),
        lambda: bwd(ls=lse.double()),                         # lse not f32
        lambda: bwd(ls=torch.zeros(12, **f32)[::2]),          # not contiguous
        lambda: bwd(ls=torch.zeros(5, **f32)),                # numel
        lambda: bwd(ls=lse.cpu()),
        # silu_mul_bwd
        lambda: C.silu_mul_bwd(torch.zeros(3, 32, **bf), gu),  # dy not halved
        lambda: C.silu_mul_bwd(torch.zeros(2, 16, **bf), gu),  # rows differ
        lambda: C.silu_mul_bwd(torch.zeros(3, 4, **bf),
                               torch.zeros(3, 8, **bf)),       # I2 % 16
        # gelu_bwd
        lambda: C.gelu_bwd(torch.zeros(16, **bf), torch.zeros(8, **bf)),
        lambda: C.gelu_bwd(torch.zeros(12, **bf), torch.zeros(12, **bf)),
        # rope
        lambda: C.rope(torch.zeros(1, 4, 2, 7, **bf),
                       torch.zeros(8, 3, **f32), torch.zeros(8, 3, **f32),
                       None, False),                           # D odd
        lambda: C.rope(x, cos.double(), sin.double(), None, False),
        lambda: C.rope(x, cos, sin.double(), None, False),     # sin not f32
        lambda: C.rope(x, torch.zeros(8, 4, **f32),
                       torch.zeros(8, 4, **f32), None, False),  # not D/2
        lambda: C.rope(x, cos, torch.zeros(9, 8, **f32), None, False),
        lambda: C.rope(x, cos.cpu(), sin.cpu(), None, False),
        lambda: C.rope(x, cos, sin, pos.cpu(), False),
        lambda: C.rope(x, torch.zeros(3, 8, **f32),
                       torch.zeros(3, 8, **f32), None, False),  # table < S
        # qkv_rope_fwd
        lambda: C.qkv_rope_fwd(qkv, cos.double(), sin.double(), None, 2, 1,
                               16),
        lambda: C.qkv_rope_fwd(qkv, torch.zeros(8, 4, **f32),
                               torch.zeros(8, 4, **f32), None, 2, 1, 16),
        lambda: C.qkv_rope_fwd(qkv, cos, torch.zeros(9, 8, **f32), None, 2,
                               1, 16),
        lambda: C.qkv_rope_fwd(qkv, cos.cpu(), sin.cpu(), None, 2, 1, 16),
        lambda: C.qkv_rope_fwd(qkv, cos, sin, pos.cpu(), 2, 1, 16),
        # qkv_rope_bwd
        lambda: C.qkv_rope_bwd(dq, dk, dk, cos.double(), sin.double(), None),
        lambda: C.qkv_rope_bwd(dq, dk, dk, torch.zeros(8, 4, **f32),
                               torch.zeros(8, 4, **f32), None),
        lambda: C.qkv_rope_bwd(dq, dk, dk, cos.cpu(), sin.cpu(), None),
        lambda: C.qkv_rope_bwd(dq, dk, dk, cos, sin, pos.long()),   # dtype
        lambda: C.qkv_rope_bwd(dq, dk, dk, cos, sin, pos[:3].contiguous()),
        lambda: C.qkv_rope_bwd(dq, dk, dk, cos, sin, pos.cpu()),
        lambda: C.qkv_rope_bwd(dq, torch.zeros(1, 3, 1, 16, **bf),
                               torch.zeros(1, 3, 1, 16, **bf), cos, sin,
                               None),                          # dk S differs
        lambda: C.qkv_rope_bwd(dq, torch.zeros(1, 4, 1, 32, **bf),
                               torch.zeros(1, 4, 1, 32, **bf), cos, sin,
                               None),                          # dk D differs
        lambda: C.qkv_rope_bwd(dq, dk, torch.zeros(1, 4, 2, 16, **bf), cos,
                               sin, None),                     # dv != dk
        # embedding
        lambda: C.embedding_fwd(table.view(-1), ids),          # table 1-D
        lambda: C.embedding_fwd(table, ids.cpu()),
        lambda: C.embedding_bwd(torch.zeros(3, 8, **bf), ids.cpu(), 5),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call #{i} was accepted")
    # the well-formed calls next to them are accepted
    torch.cuda.synchronize()
    fwd_sh()
    bwd()
    C.rope(x, cos, sin, pos, False)
    C.qkv_rope_bwd(dq, dk, dk, cos, sin, pos)
    torch.cuda.synchronize()
