"""fp64 references, inputs and bounds shared by tests/test_moe_cpu.py and
tests/test_moe_gpu.py.  Every reference takes the op's own bf16 / f32 inputs
and does all arithmetic in fp64."""
import torch

from utils_numerics import TINY, assert_bf16_close, assert_f32_close

# (T, E, k): every E the kernels are instantiated for; 8200 tokens at E = 64
# is past the router grid's 2048 blocks x 4 waves, so its loop wraps
ROUTER_SHAPES = ((70, 8, 2), (257, 64, 1), (130, 128, 8), (33, 16, 4),
                 (40, 32, 3), (8200, 64, 2))
ROUTER_RECIPES = ("plain", "dup", "masked")
# (H, k, T) of the row movers: the three widths at k = 3, then the narrowest
# row (one active lane) at k = 8, a wide row at k = 8, and k = 1 past the
# 4096 blocks x 4 waves at which the token loop wraps
ROW_CASES = ((64, 3, 70), (200, 3, 70), (2048, 3, 70), (8, 8, 70),
             (2048, 8, 33), (64, 1, 16400))

# Bound on a routing weight w_j = exp(x_j - m) / Z, relative to w_j, for an
# f32 evaluation in any order.  x_j - m is one f32 rounding of a difference
# of at most 64 in size (the test logits stay within +-32), so the exponent
# is off by at most 64 * 2^-24 = 2^-18 and exp by that much relatively, plus
# 2 ulp = 2^-23 of expf itself; that holds for the numerator and for every
# term of Z.  Z adds at most 128 positive terms: at most 127 * 2^-24 < 2^-17
# whatever the order.  The quotient rounds once more, 2^-24.  Together
# 2 * (2^-18 + 2^-23) + 2^-17 + 2^-24 < 2^-15.9; 2^-15 is taken.  TINY lets
# a weight that underflows f32's normal range lose its precision.
ROUTER_W_RTOL = 2.0 ** -15


def router_logits(T, E, k, recipe, device):
    """bf16 logits as a router GEMM leaves them (ties are frequent), plus the
    incoming d_topk_w.  'dup': every row's top-(k+1) holds one value twice
    (the two largest are made equal, and so are ranks k and k+1, so the last
    selected expert is decided by the index rule).  'masked': expert 1 sits
    at -30 everywhere and is never chosen."""
    g = torch.Generator().manual_seed(T * 1000 + E + k)
    x = (torch.randn(T, E, generator=g) * 2.0).bfloat16()
    if recipe == "dup":
        order = torch.sort(-x.float(), dim=-1, stable=True).indices
        rows = torch.arange(T)
        x[rows, order[:, 1]] = x[rows, order[:, 0]]
        if k + 1 <= E and k > 1:
            x[rows, order[:, k]] = x[rows, order[:, k - 1]]
    elif recipe == "masked":
        x[:, 1] = -30.0
    dw = torch.randn(T, k, generator=g)
    return x.to(device), dw.to(device)


def router_ref64(logits, k, norm, dw):
    """(idx int32, w, dlogits, mag of dlogits) in fp64."""
    x = logits.double()
    idx = torch.sort(-logits.float(), dim=-1, stable=True).indices[:, :k]
    if norm:
        w = torch.softmax(x.gather(1, idx), dim=-1)
        p = torch.zeros_like(x).scatter(1, idx, w)
    else:
        p = torch.softmax(x, dim=-1)
        w = p.gather(1, idx)
    g = torch.zeros_like(x).scatter(1, idx, dw.double())
    dot = (p * g).sum(-1, keepdim=True)
    mag = p * (g.abs() + (p * g.abs()).sum(-1, keepdim=True))
    return idx.to(torch.int32), w, p * (g - dot), mag


def assert_router_close(idx, w, dlogits, ref, what):
    ridx, rw, rd, rmag = ref
    assert idx.dtype == torch.int32 and torch.equal(idx, ridx), what
    assert_f32_close(w, rw, ROUTER_W_RTOL, TINY, what=what + " topk_w")
    assert_bf16_close(dlogits, rd, rmag, what + " dlogits")


def index_cases(T):
    """(name, topk_idx int32 [T, k], E): random routing, k = 1 with every
    token on one expert, and routing that leaves experts empty."""
    g = torch.Generator().manual_seed(T)
    rnd = torch.rand(T, 128, generator=g).argsort(-1)[:, :8]
    few = torch.rand(T, 16, generator=g).argsort(-1)[:, :2] * 5 + 3
    return (("random", rnd.to(torch.int32), 128),
            ("one_expert", torch.full((T, 1), 5, dtype=torch.int32), 8),
            ("empty_experts", few.to(torch.int32), 128))


def index_ref(topk_idx, E):
    flat = topk_idx.reshape(-1).long()
    order = torch.sort(flat, stable=True).indices
    dest = torch.empty_like(order)
    dest[order] = torch.arange(flat.numel())
    offs = torch.bincount(flat, minlength=E).cumsum(0)
    return dest.to(torch.int32), offs.to(torch.int32)


def rows_inputs(H, k, T, device, E=8):
    """x, sorted-layout rows yp, upstream grads and router weights for the
    row movers, with a dest from random routing."""
    g = torch.Generator().manual_seed(H + k)
    idx = torch.rand(T, E, generator=g).argsort(-1)[:, :k].to(torch.int32)
    dest = index_ref(idx, E)[0]
    bf = lambda *s: torch.randn(*s, generator=g).bfloat16().to(device)  # noqa
    return dict(k=k, dest=dest.to(device), x=bf(T, H), yp=bf(T * k, H),
                dxp=bf(T * k, H), dy=bf(T, H),
                w=torch.rand(T, k, generator=g).to(device))


def rows_ref64(inp):
    """fp64 (value, mag) pairs of the combine, the scatter's backward and
    the combine's backward."""
    k, d = inp["k"], inp["dest"].long()
    T = inp["x"].shape[0]
    w = inp["w"].double()
    yp = inp["yp"].double()[d].view(T, k, -1)
    dxp = inp["dxp"].double()[d].view(T, k, -1)
    dy = inp["dy"].double()
    terms = w.unsqueeze(-1) * yp
    dyp = torch.empty_like(inp["yp"], dtype=torch.float64)
    dyp[d] = (w.unsqueeze(-1) * dy.unsqueeze(1)).reshape(T * k, -1)
    dots = dy.unsqueeze(1) * yp
    return dict(y=(terms.sum(1), terms.abs().sum(1)),
                dx=(dxp.sum(1), dxp.abs().sum(1)), dyp=dyp,
                dw=(dots.sum(-1), dots.abs().sum(-1)))


def assert_rows_close(xp, y, dx, dyp, dw, inp, ref, what):
    H = inp["x"].shape[1]
    src = inp["x"].repeat_interleave(inp["k"], 0)
    assert torch.equal(xp[inp["dest"].long()], src), what + " xp"
    assert_bf16_close(y, *ref["y"], what + " y")
    assert_bf16_close(dx, *ref["dx"], what + " dx")
    assert_bf16_close(dyp, ref["dyp"], what=what + " dyp")
    # an H-term f32 dot product, in any order: H products and H - 1 adds,
    # each within 2^-24 of the running sum of magnitudes
    assert_f32_close(dw, ref["dw"][0], (H + 1) * 2.0 ** -24, 0.0,
                     ref["dw"][1], what + " dw")


MLP_SHAPE = dict(T=130, H=256, I=64, E=8, k=2)


def mlp_inputs(device):
    s = MLP_SHAPE
    g = torch.Generator().manual_seed(7)
    bf = lambda *sh, std=1.0: (torch.randn(*sh, generator=g) * std) \
        .bfloat16().to(device)  # noqa: E731
    return dict(x=bf(s["T"], s["H"]), router=bf(s["E"], s["H"], std=0.1),
                gate_up=bf(s["E"], 2 * s["I"], s["H"], std=0.06),
                down=bf(s["E"], s["H"], s["I"], std=0.12),
                dy=bf(s["T"], s["H"]))


MLP_TENSORS = ("x", "router", "gate_up", "down")


def mlp_run(fn, inp, k, norm):
    """(y, grads...) of fn(x, router, gate_up, down, k, norm) under the
    upstream gradient inp['dy'], all as fp64."""
    leaves = [inp[n].clone().requires_grad_() for n in MLP_TENSORS]
    y = fn(*leaves, k, norm)
    y.backward(inp["dy"].to(y.dtype))
    return [y.detach().double()] + [t.grad.double() for t in leaves]


def mlp_ref64(inp, k, norm):
    """The layer in fp64 from the same bf16 inputs.  The selection is the
    one the bf16 router logits give (an fp64 logit could order a near-tie
    the other way and route a token elsewhere); everything else, the
    weights from those logits included, is fp64."""
    idx = torch.sort(-torch.nn.functional.linear(inp["x"], inp["router"])
                     .float(), dim=-1, stable=True).indices[:, :k]
    I = MLP_SHAPE["I"]

    def layer(x, router, gate_up, down, k, norm):
        logits = x @ router.T
        w = torch.softmax(logits.gather(1, idx), -1) if norm \
            else torch.softmax(logits, -1).gather(1, idx)
        y = torch.zeros_like(x)
        for j in range(k):
            e = idx[:, j]
            h = torch.einsum("th,toh->to", x, gate_up[e])
            a = torch.nn.functional.silu(h[:, :I]) * h[:, I:]
            y = y + w[:, j:j + 1] * torch.einsum("ti,thi->th", a, down[e])
        return y

    return mlp_run(layer, {n: v.double() for n, v in inp.items()}, k, norm)
