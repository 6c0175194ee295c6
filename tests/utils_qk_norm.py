"""fp64 references, `mag` terms and the input recipe for the fused qkv split +
QK RMSNorm + RoPE op (ops/qk_norm.py, _hip/qkv_norm_rope.hip), shared by
tests/test_qk_norm_cpu.py and tests/test_qk_norm_gpu.py.  Bounds are
utils_numerics.assert_bf16_close's, unchanged.

Per q or k head row x [D], weight w, upstream gradient dout:

    r = 1/sqrt(mean(x^2) + eps)   xh = x r   y = w xh   out = Rot(y)
    dy = Rot^T(dout)   t = dy w xh   dx = r (dy w - xh mean(t))
    dw = sum over rows of dy xh

| quantity | mag                                                       |
|----------|-----------------------------------------------------------|
| forward  | |y0 c| + |y1 s|  (resp. |y0 s| + |y1 c|)                  |
| dx       | r (gm |w| + |xh| mean(gm |w| |xh|)), gm = Rot^T's two-    |
|          | product magnitude                                         |
| dw       | sum of gm |xh|                                            |

A plain module like tests/utils_numerics.py, not a conftest."""
import functools

import torch

from utils_numerics import f32r, rope_positions, rope_ref64, truncate_to_bf16

EPS = 1e-6
THETA = 1e6
MAX_POS = 2048  # > S + 8 for every CPU / binding shape that uses positions

# (B, S, Hq, Hkv, D): one token row of three heads; two D = 64 / D = 128
# shapes whose 10 / 12 head rows per token leave a wave pass partly idle
SHAPES = ((1, 3, 1, 1, 64), (2, 33, 8, 2, 64), (2, 33, 8, 2, 128))


def qk_inputs(B, S, Hq, Hkv, D, device="cpu", seed=0):
    """dict(qkv [B,S,W], wq, wk [D], dq, dk, dv) in bf16.  Token 0's q head
    0 is a zero row, its k head 0 carries one 300.0 outlier, token 1's q
    head 0 is scaled by 2^-20; both weights have a zero and a negative
    entry."""
    g = torch.Generator(device="cpu").manual_seed(seed * 101 + D + S)
    HA = Hq + 2 * Hkv
    qkv = torch.randn(B, S, HA, D, generator=g)
    qkv[0, 0, 0] = 0.0
    qkv[0, 0, Hq, 5] = 300.0
    qkv[0, 1, 0] *= 2.0 ** -20
    wq = 1.0 + 0.5 * torch.randn(D, generator=g)
    wk = 1.0 + 0.5 * torch.randn(D, generator=g)
    wq[3], wq[D // 2 + 1] = 0.0, -wq[D // 2 + 1].abs() - 0.25
    wk[D - 1], wk[2] = 0.0, -wk[2].abs() - 0.25
    out = dict(
        qkv=qkv.view(B, S, HA * D), wq=wq, wk=wk,
        dq=torch.randn(B, S, Hq, D, generator=g),
        dk=torch.randn(B, S, Hkv, D, generator=g),
        dv=torch.randn(B, S, Hkv, D, generator=g))
    return {k: v.bfloat16().to(device) for k, v in out.items()}


def tables(D, max_pos, device):
    """The project's own f32 cos / sin tables (what the kernel reads)."""
    from distributed_training_guide_amd.ops.reference import rope_tables

    return rope_tables(D, max_pos, THETA, device=device)


def _split(inp, Hq, Hkv, D):
    B, S, _ = inp["qkv"].shape
    q, k, v = inp["qkv"].split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    return (q.reshape(B, S, Hq, D), k.reshape(B, S, Hkv, D),
            v.reshape(B, S, Hkv, D))


def _rows_ref64(x, w, dout, cos, sin, positions, eps):
    """One of q / k: (out, out_mag, dx, dx_mag, dw, dw_mag), all fp64."""
    x = x.double()
    w = w.double()
    r = 1.0 / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh = x * r
    out, out_mag = rope_ref64(w * xh, cos, sin, positions)
    dy, gm = rope_ref64(dout, cos, sin, positions, backward=True)
    t = dy * w * xh
    dx = r * (dy * w - xh * t.mean(-1, keepdim=True))
    dx_mag = r * (gm * w.abs() + xh.abs() *
                  (gm * w.abs() * xh.abs()).mean(-1, keepdim=True))
    D = x.shape[-1]
    dw = (dy * xh).reshape(-1, D).sum(0)
    dw_mag = (gm * xh.abs()).reshape(-1, D).sum(0)
    return out, out_mag, dx, dx_mag, dw, dw_mag


def qk_ref64(inp, Hq, Hkv, D, cos, sin, positions=None, eps=EPS):
    """fp64 reference of forward and backward from the bf16 inputs, computed
    on the inputs' device.  eps is the f32 value the binding hands the
    kernel.  Keys: q, k, dqkv, dwq, dwk with their *_mag, and v (exact)."""
    eps = f32r(eps)
    B, S, _ = inp["qkv"].shape
    xq, xk, v = _split(inp, Hq, Hkv, D)
    q, qm, dxq, dxqm, dwq, dwqm = _rows_ref64(xq, inp["wq"], inp["dq"], cos,
                                              sin, positions, eps)
    k, km, dxk, dxkm, dwk, dwkm = _rows_ref64(xk, inp["wk"], inp["dk"], cos,
                                              sin, positions, eps)
    dv = inp["dv"].double()
    dqkv = torch.cat([dxq.reshape(B, S, -1), dxk.reshape(B, S, -1),
                      dv.reshape(B, S, -1)], dim=-1)
    dqkv_mag = torch.cat([dxqm.reshape(B, S, -1), dxkm.reshape(B, S, -1),
                          dv.abs().reshape(B, S, -1)], dim=-1)
    return dict(q=q, q_mag=qm, k=k, k_mag=km, v=v.contiguous(),
                dqkv=dqkv, dqkv_mag=dqkv_mag, dwq=dwq, dwq_mag=dwqm,
                dwk=dwk, dwk_mag=dwkm)


@functools.lru_cache(maxsize=None)
def cpu_case(shape, with_positions):
    """(inputs, cos, sin, positions, reference) on the CPU, computed once per
    (shape, positions) and shared; nothing in it is modified by a test."""
    B, S, Hq, Hkv, D = shape
    inp = qk_inputs(B, S, Hq, Hkv, D)
    cos, sin = tables(D, MAX_POS, "cpu")
    pos = rope_positions(S, MAX_POS, "cpu") if with_positions else None
    return inp, cos, sin, pos, qk_ref64(inp, Hq, Hkv, D, cos, sin, pos)


# --------------------------------------------------------------------------
# an f32 evaluation of the same formulas, and what a subtly wrong kernel
# would compute instead
# --------------------------------------------------------------------------
DAMAGES = ("no_eps", "rotate_first", "mean_without_weight", "dw_row_dropped",
           "truncate")


def _rot32(x, cos, sin, positions, backward=False):
    S, D = x.shape[1], x.shape[-1]
    idx = torch.arange(S) if positions is None else positions.long()
    c = cos[idx].view(1, S, 1, D // 2)
    s = sin[idx].view(1, S, 1, D // 2)
    x0, x1 = x[..., :D // 2], x[..., D // 2:]
    if backward:
        return torch.cat([x0 * c + x1 * s, -x0 * s + x1 * c], -1)
    return torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], -1)


def _rows_f32(x, w, dout, cos, sin, positions, eps, damage):
    x, w, dout = x.float(), w.float(), dout.float()
    D = x.shape[-1]
    ms = x.pow(2).mean(-1, keepdim=True)
    if damage == "no_eps":
        r = torch.rsqrt(ms)
    else:
        r = torch.rsqrt(ms + torch.tensor(eps, dtype=torch.float32))
    if damage == "rotate_first":
        out = w * (_rot32(x, cos, sin, positions) * r)
    else:
        out = _rot32(w * (x * r), cos, sin, positions)
    xh = x * r
    dy = _rot32(dout, cos, sin, positions, backward=True)
    t = dy * xh if damage == "mean_without_weight" else dy * w * xh
    dx = r * (dy * w - xh * t.mean(-1, keepdim=True))
    rows = (dy * xh).reshape(-1, D)
    if damage == "dw_row_dropped":
        rows = rows[:-1]
    # serial f32 accumulation in row order
    dw = torch.zeros(D, dtype=torch.float32)
    for chunk in rows.split(4096):
        dw = dw + chunk.cumsum(0, dtype=torch.float32)[-1]
    return out, dx, dw


def qk_eval_f32(inp, Hq, Hkv, D, cos, sin, positions=None, eps=EPS,
                damage=None):
    """CPU f32 evaluation with one rounding to bf16 at the end; `damage`
    (one of DAMAGES) computes what a wrong kernel would.  Same keys as
    qk_ref64 without the mags."""
    assert damage is None or damage in DAMAGES, damage
    eps = f32r(eps)
    B, S, _ = inp["qkv"].shape
    xq, xk, v = _split(inp, Hq, Hkv, D)
    q, dxq, dwq = _rows_f32(xq, inp["wq"], inp["dq"], cos, sin, positions,
                            eps, damage)
    k, dxk, dwk = _rows_f32(xk, inp["wk"], inp["dk"], cos, sin, positions,
                            eps, damage)
    dqkv = torch.cat([dxq.reshape(B, S, -1), dxk.reshape(B, S, -1),
                      inp["dv"].float().reshape(B, S, -1)], dim=-1)
    rnd = truncate_to_bf16 if damage == "truncate" else \
        (lambda t: t.bfloat16())
    return dict(q=rnd(q), k=rnd(k), v=v.contiguous(), dqkv=rnd(dqkv),
                dwq=rnd(dwq), dwk=rnd(dwk))


CHECKED = (("q", "q_mag"), ("k", "k_mag"), ("dqkv", "dqkv_mag"),
           ("dwq", "dwq_mag"), ("dwk", "dwk_mag"))


def assert_qk_close(got, ref, what=""):
    """Every element of q, k, dqkv, dwq and dwk inside assert_bf16_close's
    bound; v and the dv segment of dqkv bit-exact."""
    from utils_numerics import assert_bf16_close

    for key, mag in CHECKED:
        if key in got:
            assert_bf16_close(got[key], ref[key], ref[mag], f"{what} {key}")
    if "v" in got:
        assert torch.equal(got["v"], ref["v"].to(got["v"].device)), \
            f"{what} v is not a bit-exact copy"
