"""Per-element numeric checks for the streaming kernels: the checker, plain
fp64 references and the input recipes shared by the CPU proof
(tests/test_numerics_helper_cpu.py) and the GPU tests
(tests/test_streaming_ops_gpu.py, tests/test_ce_sharded_gpu.py).

Every reference takes the kernel's own bf16 / f32 inputs, upcasts them to
fp64 and does all arithmetic there.  Where the result is a sum of terms that
can cancel, the reference also returns `mag`: the sum of the absolute values
of those terms, which is what an f32 evaluation's rounding error scales
with.  A plain module like tests/utils_dist.py, not a conftest."""
import math

import numpy as np
import torch

IGNORE_INDEX = -100

# Smallest normal number of bf16 AND of f32 (both have an 8-bit exponent).
# Below it neither format keeps its relative precision: exp(-96) * 96 is
# 2e-40, which f32 cannot form at all because exp(96) overflows, and a
# softmax probability of exp(-100) is a 1-bit f32 denormal.  A correct f32
# implementation therefore errs by up to one such number on results that
# underflow, and the bounds below allow exactly that and nothing more.
TINY = 2.0 ** -126

GELU_K = math.sqrt(2.0 / math.pi)
GELU_C = 0.044715


# --------------------------------------------------------------------------
# the checker
# --------------------------------------------------------------------------
def _check(y, ref64, bound64, what, kind):
    assert y.shape == ref64.shape, \
        f"{what}: shape {tuple(y.shape)} vs reference {tuple(ref64.shape)}"
    ref64 = ref64.to(y.device)
    bound64 = bound64.to(y.device)
    y64 = y.detach().to(torch.float64)
    fin_r = torch.isfinite(ref64)
    fin_y = torch.isfinite(y64)
    # non-finite values match exactly: same places, same sign of infinity,
    # NaN only where the reference has NaN
    same_nonfinite = (y64 == ref64) | (torch.isnan(y64) & torch.isnan(ref64))
    err = (y64 - ref64).abs()
    bad = torch.where(fin_r & fin_y, err > bound64, ~same_nonfinite)
    nbad = int(bad.sum().item())
    if nbad == 0:
        return
    # worst finite excess, or the first non-finite mismatch
    score = torch.where(fin_r & fin_y, err - bound64,
                        torch.full_like(err, float("inf")))
    score = torch.where(bad, score, torch.full_like(err, -float("inf")))
    flat = int(score.reshape(-1).argmax().item())
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(y.shape))) \
        if y.dim() else ()
    raise AssertionError(
        f"{what or 'tensor'} [{kind}]: {nbad} of {y.numel()} elements out of "
        f"bound; worst at {idx}: got {y64.reshape(-1)[flat].item()!r}, "
        f"reference {ref64.reshape(-1)[flat].item()!r}, "
        f"|diff| {err.reshape(-1)[flat].item():.6e}, "
        f"bound {bound64.reshape(-1)[flat].item():.6e}")


def assert_bf16_close(y, ref64, mag64=None, what=""):
    """Every element of the bf16 kernel output `y` satisfies

        |y - ref| <= 2^-8 * |ref| + 2^-16 * mag + 2^-126

    against the fp64 reference `ref64` computed from the same bf16 inputs.
    `mag64` is the fp64 sum of the absolute values of the terms the kernel
    adds to form the element (default |ref64|).  No element is exempt.

    Derivation.  bf16 carries 8 significant bits, so round-to-nearest of a
    value x errs by at most half an ulp, which is at most 2^-8 * |x|.  The
    second term allows the f32 evaluation (__expf and tanhf included) 256
    f32 ulps of the largest intermediate before that rounding: far above
    anything these kernels do, far below one bf16 ulp.  The last term is the
    smallest normal number of both formats (see TINY): results that
    underflow below it carry no relative precision in f32 or bf16.

    Non-finite values must match exactly (same positions, same sign of
    infinity); NaN or inf in `y` where the reference is finite fails."""
    assert y.dtype == torch.bfloat16, f"{what}: expected bf16, got {y.dtype}"
    assert ref64.dtype == torch.float64
    mag = ref64.abs() if mag64 is None else mag64.to(torch.float64)
    bound = 2.0 ** -8 * ref64.abs() + 2.0 ** -16 * mag + TINY
    bound = torch.where(torch.isfinite(bound), bound, torch.zeros_like(bound))
    _check(y, ref64, bound, what, "bf16")


def assert_f32_close(y, ref64, rtol, atol, mag64=None, what=""):
    """Every element of the f32 output `y` satisfies
    |y - ref| <= rtol * mag + atol (mag defaults to |ref|), with the same
    report and the same treatment of non-finite values as
    assert_bf16_close."""
    assert y.dtype == torch.float32, f"{what}: expected f32, got {y.dtype}"
    assert ref64.dtype == torch.float64
    mag = ref64.abs() if mag64 is None else mag64.to(torch.float64)
    bound = rtol * mag + atol
    bound = torch.where(torch.isfinite(bound), bound, torch.zeros_like(bound))
    _check(y, ref64, bound, what, "f32")


# --------------------------------------------------------------------------
# damage: what a subtly wrong kernel would produce
# --------------------------------------------------------------------------
def bump_bf16_ulps(y, index, ulps):
    """Copy of bf16 `y` with element `index` moved by `ulps` bf16 ulps away
    from zero."""
    out = y.clone()
    bits = out.view(torch.int16)
    bits[index] += ulps
    return out


def truncate_to_bf16(f32):
    """bf16 by truncation (low 16 bits masked) instead of round-to-nearest."""
    bits = f32.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).bfloat16()


# --------------------------------------------------------------------------
# silu_mul
# --------------------------------------------------------------------------
SILU_PINNED = (0.0, 88.0, -88.0, 96.0, -96.0)  # bf16-exact gate values


def silu_inputs(rows, I, device, seed=0):
    """gu [rows, 2I] bf16 with gates uniform in +-30 and the first columns
    of every row pinned to SILU_PINNED, plus an upstream dy [rows, I]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    gate = (torch.rand(rows, I, generator=g) * 60.0 - 30.0)
    up = torch.randn(rows, I, generator=g)
    n = min(I, len(SILU_PINNED))
    gate[:, :n] = torch.tensor(SILU_PINNED[:n])
    if I >= 16:  # and once more at the end of the row
        gate[:, I - n:] = torch.tensor(SILU_PINNED[:n])
    gu = torch.cat([gate, up], dim=-1).bfloat16().to(device)
    dy = torch.randn(rows, I, generator=g).bfloat16().to(device)
    return gu, dy


def silu_mul_ref64(gu):
    I = gu.shape[-1] // 2
    x = gu[..., :I].double()
    u = gu[..., I:].double()
    sig = 1.0 / (1.0 + torch.exp(-x))
    return x * sig * u


def silu_mul_bwd_ref64(dy, gu):
    """(dg, mag_dg, du): dg = dy*u*sig*(1 + x*(1-sig)); the bracket cancels
    for negative x."""
    I = gu.shape[-1] // 2
    x = gu[..., :I].double()
    u = gu[..., I:].double()
    d = dy.double()
    sig = 1.0 / (1.0 + torch.exp(-x))
    t = x * (1.0 - sig)
    dg = d * u * sig * (1.0 + t)
    mag = (d * u * sig).abs() * (1.0 + t.abs())
    du = d * x * sig
    return dg, mag, du


# --------------------------------------------------------------------------
# rope (rotate-half, pairs (i, i + D/2)) on the project's own f32 table
# --------------------------------------------------------------------------
def rope_ref64(x, cos, sin, positions=None, backward=False):
    """x [B,S,H,D]; cos/sin f32 [max_pos, D/2].  Returns (y, mag), mag the
    sum of the two products' absolute values."""
    B, S, H, D = x.shape
    h = D // 2
    idx = torch.arange(S, device=x.device) if positions is None \
        else positions.long()
    c = cos[idx].double().view(1, S, 1, h)
    s = sin[idx].double().view(1, S, 1, h)
    x0 = x[..., :h].double()
    x1 = x[..., h:].double()
    if backward:
        y0, y1 = x0 * c + x1 * s, -x0 * s + x1 * c
    else:
        y0, y1 = x0 * c - x1 * s, x0 * s + x1 * c
    m0 = (x0 * c).abs() + (x1 * s).abs()
    m1 = (x0 * s).abs() + (x1 * c).abs()
    return torch.cat([y0, y1], -1), torch.cat([m0, m1], -1)


# backward(forward(x)) against x itself.  y = forward(x) carries a rounding
# of at most 2^-8 |y| per element; the inverse rotation turns that into at
# most 2^-8 (|c| |y0| + |s| |y1|) = 2^-8 * mag of the backward pass, on top
# of the backward's own bound 2^-8 |ref| + 2^-16 mag with
# |ref| <= |x| + 2^-8 mag.  As assert_bf16_close multiplies mag by 2^-16
# this is mag * (2^8 + 2).
ROPE_ROUND_TRIP = 258.0


def rope_positions(S, max_pos, device):
    """Non-monotone int32 positions with repeats and an offset; the largest
    is max_pos - 1 > S."""
    assert max_pos > S + 8
    p = (torch.arange(S) * 7 + 5) % (max_pos - 1)
    p[0] = max_pos - 1
    if S > 2:
        p[2] = p[1]          # repeat
        p[S - 1] = 0
    return p.to(torch.int32).to(device)


# --------------------------------------------------------------------------
# causal cross entropy, per row
# --------------------------------------------------------------------------
CE_RECIPES = ("normal", "offset", "dominant_label", "dominant_other",
              "neginf")


def ce_labels(B, S, V, seed=0):
    """Labels on columns 0 and V-1, several ignored positions and, with
    B > 1, one batch row entirely ignored."""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    lab = torch.randint(0, V, (B, S), generator=g)
    if S >= 6:
        lab[0, 1] = 0
        lab[0, 2] = V - 1
        lab[:, 3::5] = IGNORE_INDEX
    else:  # a single loss row or two: alternate the two edge columns
        lab[0, 1] = (V - 1) if seed % 2 == 0 else 0
    if B > 1:
        lab[B - 1] = IGNORE_INDEX
    return lab


def ce_sharded_labels(B, S, V, tp, owners=None, seed=0):
    """Labels for a vocab split into `tp` contiguous shards: both sides of
    every boundary between label-owning shards (r*Vl - 1 and r*Vl), ignored
    positions, and with owners < tp no label at all in the last shards."""
    owners = tp if owners is None else owners
    Vl = V // tp
    g = torch.Generator(device="cpu").manual_seed(2000 + seed)
    lab = torch.randint(0, owners * Vl, (B, S), generator=g)
    edge = [c for r in range(1, owners) for c in (r * Vl - 1, r * Vl)]
    edge += [0, owners * Vl - 1]
    free = [s for s in range(1, S) if s % 5 != 3]
    assert len(edge) <= len(free)
    for s, c in zip(free, edge):
        lab[0, s] = c
    lab[:, 3::5] = IGNORE_INDEX
    return lab


def ce_neginf_columns(V):
    """Masked columns: column 0, a column that opens its 8-lane vector with
    finite logits after it, one in mid-vector, and from V = 32 on the whole
    leading 16-column block."""
    cols = {0, V // 2 + 1}
    if V >= 32:
        cols |= set(range(16)) | {24}
    return sorted(cols)


def ce_inputs(B, S, V, recipe, device, seed=0):
    """(logits bf16 [B,S,V], labels int64 [B,S]) for one recipe."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, S, V, generator=g)
    lab = ce_labels(B, S, V, seed)
    tgt = lab[:, 1:]                      # label of logits row (b, s)
    valid = tgt != IGNORE_INDEX
    if recipe == "offset":
        off = torch.tensor([200.0, -200.0, 0.0])[torch.arange(B * S) % 3]
        x = x + off.view(B, S, 1)
    elif recipe in ("dominant_label", "dominant_other"):
        col = tgt.clamp_min(0)
        if recipe == "dominant_other":
            col = (col + 1) % V
        hot = torch.zeros(B, S - 1, V, dtype=torch.bool)
        hot.scatter_(2, col.unsqueeze(-1), valid.unsqueeze(-1))
        x[:, :-1][hot] = 100.0
    elif recipe == "neginf":
        cols = ce_neginf_columns(V)
        x[..., cols] = -float("inf")
        masked = torch.zeros(V, dtype=torch.bool)
        masked[cols] = True
        move = (lab != IGNORE_INDEX) & masked[lab.clamp_min(0)]
        lab[move] = V - 2                 # a finite column
        assert not masked[V - 2] and not masked[V - 1]
    else:
        assert recipe == "normal", recipe
    return x.bfloat16().to(device), lab.to(device)


def ce_ref64(logits, labels, ignore_index=IGNORE_INDEX):
    """Per loss row r = b*(S-1)+s: lse, loss, the label's logit and the
    softmax, all fp64.  Ignored rows carry loss 0 and lse -inf, as the
    kernel marks them."""
    B, S, V = logits.shape
    x = logits[:, :-1].double().reshape(B * (S - 1), V)
    tgt = labels[:, 1:].reshape(-1)
    valid = tgt != ignore_index
    lse = torch.logsumexp(x, dim=-1)
    p = torch.exp(x - lse.unsqueeze(-1))
    xl = x.gather(1, tgt.clamp_min(0).unsqueeze(-1)).squeeze(-1)
    xl = torch.where(valid, xl, torch.zeros_like(xl))
    ninf = torch.full_like(lse, -float("inf"))
    return dict(
        lse=torch.where(valid, lse, ninf),
        lse_all=lse,
        loss=torch.where(valid, lse - xl, torch.zeros_like(lse)),
        x_label=xl, p=p, valid=valid, target=tgt,
        n_valid=int(valid.sum().item()))


def ce_row_mag(ref):
    """|lse| + |x_label| per row (0 on ignored rows)."""
    lse = torch.where(ref["valid"], ref["lse_all"].abs(),
                      torch.zeros_like(ref["lse_all"]))
    return lse + ref["x_label"].abs()


CE_ROW_RTOL = 2.0 ** -21
CE_ROW_ATOL = 2e-5


def ce_dlogits_ref64(logits, ref, scale, label_shift=0):
    """(dlogits, mag) [B,S,V]: scale * (p - onehot) on loss rows, zero on
    ignored rows and on every batch row's last position;
    mag = scale * (p + onehot).  label_shift moves the one-hot (damage)."""
    B, S, V = logits.shape
    p = ref["p"]
    onehot = torch.zeros_like(p)
    col = (ref["target"].clamp_min(0) + label_shift) % V
    onehot.scatter_(1, col.unsqueeze(-1), 1.0)
    v = ref["valid"].unsqueeze(-1).double()
    d = torch.zeros(B, S, V, dtype=torch.float64, device=logits.device)
    m = torch.zeros_like(d)
    d[:, :-1] = (scale * (p - onehot) * v).view(B, S - 1, V)
    m[:, :-1] = (abs(scale) * (p + onehot) * v).view(B, S - 1, V)
    return d, m


def ce_online_f32(logits):
    """CPU f32 emulation of ce_fwd_kernel's arithmetic on logits[:, :-1]:
    256 threads, each folding its 8-wide vectors in order with the online
    max / rescaled-sum update, then max-combine and rescaled sum.  Returns
    f32 lse per loss row."""
    B, S, V = logits.shape
    assert V % 8 == 0
    x = logits[:, :-1].float().reshape(B * (S - 1), V)
    n = x.shape[0]
    stride = 256 * 8
    passes = (V + stride - 1) // stride
    pad = torch.full((n, passes * stride), -float("inf"))
    pad[:, :V] = x
    lanes = pad.view(n, passes, 256, 8)
    ninf = -float("inf")
    m = torch.full((n, 256), ninf)
    s = torch.zeros(n, 256)
    for k in range(passes):
        for j in range(8):
            f = lanes[:, k, :, j]
            live = f != ninf
            up = live & (f > m)
            s = torch.where(up, s * torch.exp(m - f), s)
            m = torch.where(up, f, m)
            s = torch.where(live, s + torch.exp(f - m), s)
    gm = m.amax(dim=1, keepdim=True)
    s = torch.where(m == ninf, torch.zeros_like(s), s * torch.exp(m - gm))
    return gm.squeeze(1) + torch.log(s.sum(dim=1))


# Bound on a shard's sumout = sum(exp(x - max)) against fp64, relative (the
# sum is >= 1, its largest term being exp(0)).  Terms that matter have
# |x - max| <= 20, so __expf's argument scaling errs by about 20 * 2^-24 in
# relative terms; the adds are a chain of at most 24 per thread (3 passes of
# 8 at V_local = 2080) plus 6 wave and 2 block folding steps, each 2^-24.
# Together under 52 * 2^-24 < 2^-18.
CE_SUM_RTOL = 2.0 ** -18


def ce_shard_sum_ref64(shard):
    """fp64 sum(exp(x - max)) per loss row of a [B,S,V_local] shard."""
    B, S, V = shard.shape
    x = shard[:, :-1].double().reshape(B * (S - 1), V)
    return torch.exp(x - x.amax(dim=-1, keepdim=True)).sum(dim=-1)


# --------------------------------------------------------------------------
# tanh-GELU
# --------------------------------------------------------------------------
GELU_PINNED = (0.0, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 9.0, -9.0, 40.0, -40.0)


def gelu_inputs(numel, device, seed=0):
    """x uniform in +-12 with a leading block pinned to GELU_PINNED (where
    1 + tanh cancels or saturates), plus an upstream dy."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(numel, generator=g) * 24.0 - 12.0
    n = min(numel, len(GELU_PINNED))
    x[:n] = torch.tensor(GELU_PINNED[:n])
    if numel >= 64:  # every pinned value, also away from the first vector
        x[numel - 16:numel - 16 + len(GELU_PINNED)] = \
            torch.tensor(GELU_PINNED)
    dy = torch.randn(numel, generator=g)
    return x.bfloat16().to(device), dy.bfloat16().to(device)


def gelu_ref64(x):
    """(y, mag) with mag = |0.5 x| * (1 + |t|)."""
    f = x.double()
    t = torch.tanh(GELU_K * (f + GELU_C * f ** 3))
    return 0.5 * f * (1.0 + t), (0.5 * f).abs() * (1.0 + t.abs())


def gelu_bwd_ref64(dy, x):
    """(dx, mag): dx = dy * (0.5 (1+t) + 0.5 x (1-t^2) u'); mag sums the two
    derivative terms' absolute values, the first as 0.5 (1 + |t|)."""
    f = x.double()
    t = torch.tanh(GELU_K * (f + GELU_C * f ** 3))
    du = GELU_K * (1.0 + 3.0 * GELU_C * f * f)
    a = 0.5 * (1.0 + t)
    b = 0.5 * f * (1.0 - t * t) * du
    d = dy.double()
    return d * (a + b), d.abs() * (0.5 * (1.0 + t.abs()) + b.abs())


# --------------------------------------------------------------------------
# AdamW: one step from a known state
# --------------------------------------------------------------------------
ADAMW_SIZES = (1, 7, 8, 9, 18315, 262144, 262155)
ADAMW_HYPER = (
    dict(lr=1e-2, weight_decay=0.1, betas=(0.9, 0.95), eps=1e-8),
    dict(lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8),  # defaults
)


def f32r(v):
    """The value a Python float takes when the binding casts it to float."""
    return float(np.float32(v))


def adamw_f32_hyper(h):
    """The same hyperparameters rounded to f32: what the kernel receives."""
    return dict(lr=f32r(h["lr"]), weight_decay=f32r(h["weight_decay"]),
                betas=(f32r(h["betas"][0]), f32r(h["betas"][1])),
                eps=f32r(h["eps"]))


def adamw_state(n, p_dtype, g_dtype, device, seed=0):
    """(p, g, exp_avg, exp_avg_sq) with non-zero moments, exp_avg_sq >= 0."""
    gen = torch.Generator(device="cpu").manual_seed(seed * 7919 + n)
    p = torch.randn(n, generator=gen).to(p_dtype).to(device)
    g = torch.randn(n, generator=gen).to(g_dtype).to(device)
    m = (0.1 * torch.randn(n, generator=gen)).to(device)
    v = (0.1 * torch.randn(n, generator=gen)).square().to(device)
    return p, g, m, v


def adamw_ref64(p, g, m, v, hyper, step):
    """One AdamW step in fp64 from the f32-rounded constants the binding
    hands the kernel.  Returns a dict of (ref, mag) pairs for p, m, v and
    the update delta."""
    h = adamw_f32_hyper(hyper)
    lr, wd, eps = h["lr"], h["weight_decay"], h["eps"]
    b1, b2 = h["betas"]
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = torch.sqrt(v1 / bc2) + eps
    delta = lr * (m1 / bc1) / denom
    p1 = p * (1.0 - lr * wd) - delta
    # the update inherits the rounding of exp_avg, which scales with the
    # magnitudes of its two terms and not with their (possibly cancelling)
    # sum: delta_mag is delta evaluated on those magnitudes, equal to
    # |delta| wherever beta1*m and (1-beta1)*g agree in sign
    m_mag = b1 * m.abs() + (1.0 - b1) * g.abs()
    delta_mag = lr * (m_mag / bc1) / denom
    return dict(
        p=p1, delta=delta, delta_mag=delta_mag,
        p_mag=p.abs() + delta_mag,
        m=m1, m_mag=m_mag,
        v=v1, v_mag=b2 * v.abs() + (1.0 - b2) * g * g)


def set_grad(p, g):
    """p.grad = g, also where the dtypes differ (as parallel/fsdp.py does
    for reduce_dtype=fp32)."""
    if g.dtype != p.dtype:
        p.grad_dtype = g.dtype
    p.grad = g


def adamw_one_step(opt_cls, hyper, k, p_dtype, g_dtype, sizes, device,
                   f32_hyper=False):
    """Step k of one optimizer holding a parameter per size, from a written
    state; returns [(p, exp_avg, exp_avg_sq, ref)].  f32_hyper hands the
    optimizer the constants already rounded to f32: the eager path keeps
    Python doubles, the kernel receives floats."""
    h = adamw_f32_hyper(hyper) if f32_hyper else hyper
    params, starts = [], []
    for n in sizes:
        p, g, m, v = adamw_state(n, p_dtype, g_dtype, device)
        starts.append((p.clone(), g.clone(), m.clone(), v.clone()))
        p = torch.nn.Parameter(p)
        set_grad(p, g)
        params.append(p)
    opt = opt_cls(params, **h)
    for p, (_, _, m, v) in zip(params, starts):
        opt.state[p]["exp_avg"] = m.clone()
        opt.state[p]["exp_avg_sq"] = v.clone()
    opt.param_groups[0]["step"] = k - 1
    opt.step()
    return [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"],
             adamw_ref64(*st, hyper, k)) for p, st in zip(params, starts)]


def assert_adamw_close(p, m, v, ref, what=""):
    """fp32 p within 2^-22 |p_ref| + 2^-20 delta_mag, bf16 p by
    assert_bf16_close with mag = |p| + delta_mag, moments within rtol 2^-21
    of the sum of their two terms' magnitudes.

    delta_mag (see adamw_ref64) is |delta| except where exp_avg's two terms
    cancel.  With plain |delta| the eager f32 step itself misses the fp32
    bound there: 1 element of 262155 at lr=1e-2, betas=(0.9, 0.95), step 1,
    |diff| 4.52e-10 against 4.47e-10."""
    assert_f32_close(m, ref["m"], 2.0 ** -21, 0.0, ref["m_mag"],
                     what + " exp_avg")
    assert_f32_close(v, ref["v"], 2.0 ** -21, 0.0, ref["v_mag"],
                     what + " exp_avg_sq")
    if p.dtype == torch.bfloat16:
        assert_bf16_close(p, ref["p"], ref["p_mag"], what + " p")
    else:
        bound_mag = 2.0 ** -22 * ref["p"].abs() + 2.0 ** -20 * ref["delta_mag"]
        assert_f32_close(p, ref["p"], 1.0, 0.0, bound_mag, what + " p")


# --------------------------------------------------------------------------
# embedding
# --------------------------------------------------------------------------
def embedding_inputs(V, H, ids_shape, device, seed=0, all_equal=False):
    """(table bf16 [V,H], ids int64, dy bf16 ids_shape+[H]).  dy is drawn
    from {k/64 : k in [-128,128]}, so every f32 partial sum of up to 33000
    of them is exact in any order: |sum| * 64 <= 128 * 33000 < 2^24."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    table = torch.randn(V, H, generator=g).bfloat16()
    if all_equal:
        ids = torch.full(ids_shape, V // 2, dtype=torch.int64)
    else:
        ids = torch.randint(0, V, ids_shape, generator=g)
    k = torch.randint(-128, 129, (*ids_shape, H), generator=g)
    dy = (k.float() / 64.0).bfloat16()
    assert torch.equal(dy.float() * 64.0, k.float())
    return table.to(device), ids.to(device), dy.to(device)


def embedding_bwd_ref(dy, ids, V):
    """The fp64 scatter sum rounded once to bf16: the only correct answer
    for embedding_inputs' dy."""
    H = dy.shape[-1]
    acc = torch.zeros(V, H, dtype=torch.float64, device=dy.device)
    acc.index_add_(0, ids.reshape(-1), dy.reshape(-1, H).double())
    return acc.bfloat16()
