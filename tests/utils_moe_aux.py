"""fp64 reference and bounds for the router's auxiliary losses, shared by
tests/test_moe_aux_cpu.py and tests/test_moe_aux_gpu.py."""
import torch

from utils_numerics import assert_bf16_close, assert_f32_close

# The aux grid's cap (MRA_GRID_CAP in _hip/moe_router_aux.hip) x 4 waves x
# tokens per wave (64 / E below 64 experts), plus one: the smallest T at which
# the token loop wraps and every block writes a partial row.
AUX_GRID_CAP = 512
WRAP_T = {8: AUX_GRID_CAP * 4 * 8 + 1, 128: AUX_GRID_CAP * 4 + 1}
# (T, E, k): every instantiated E, k = 1 and k = 8, T = 1, a ragged last wave
# (70 tokens, 8 to a wave), and the two wrapping sizes
AUX_SHAPES = ((70, 8, 2), (1, 16, 1), (40, 32, 8), (257, 64, 3),
              (130, 128, 8), (WRAP_T[8], 8, 2), (WRAP_T[128], 128, 8))

# A full-softmax probability p = exp(x - m) * (1 / Z) in f32.  As derived for
# ROUTER_W_RTOL (utils_moe.py) every exp term is off by at most 2^-18 + 2^-23
# relatively and the row sum adds 2^-17, so Z is within 2^-16.4; the
# reciprocal and the product round once each: p is within 2^-15.97.  aux sums
# non-negative terms c[e] * p[t, e], so a relative bound holds: a lane's f32
# chain over its tokens (at most 16 trips of the token loop here, 2 in these
# shapes) and the 5 fold steps add 21 * 2^-24, the rest is double and one
# final rounding.  Below 2^-15.8; 2^-15 is taken.
AUX_RTOL = 2.0 ** -15
# lse = m + log(Z): log turns Z's relative 2^-16.4 into an absolute error,
# logf and the add round relative to s = |m| + |log Z|: within
# 2^-16 + 2^-22 * s of fp64.  lse^2 is then off by 2 * s times that, and the
# f32 square and sum (same chain as above) by 2^-19 * s^2.
LSE_ATOL, LSE_RTOL, ZSUM_RTOL = 2.0 ** -16, 2.0 ** -22, 2.0 ** -19


def aux_ref64(logits, k, norm, dw, g_aux, g_z):
    """The definitions in fp64 from the bf16 logits, the selection taken
    from the f32 logits: idx, counts, aux, z, z's bound, dlogits and the
    summed magnitudes of dlogits' three terms."""
    x = logits.detach().cpu().double().requires_grad_()
    T, E = x.shape
    idx = torch.sort(-x.detach().float(), dim=-1, stable=True).indices[:, :k]
    full = torch.softmax(x, -1)
    w = torch.softmax(x.gather(1, idx), -1) if norm else full.gather(1, idx)
    lse = torch.logsumexp(x, -1)
    counts = torch.bincount(idx.reshape(-1), minlength=E)
    aux = E * (counts.double() / T * full.mean(0)).sum()
    z = lse.square().mean()
    dw = dw.cpu().double()
    ((w * dw).sum() + g_aux * aux + g_z * z).backward()
    with torch.no_grad():
        m = x.amax(-1)
        s = m.abs() + (lse - m).abs()
        z_bound = (2 * s * (LSE_ATOL + LSE_RTOL * s) + ZSUM_RTOL * s * s).mean()
        pr = torch.zeros_like(x).scatter(1, idx, w) if norm else full
        g = torch.zeros_like(x).scatter(1, idx, dw).abs()
        a = (abs(g_aux) * E * counts.double() / T ** 2).expand_as(x)
        mag = pr * (g + (pr * g).sum(-1, keepdim=True)) \
            + full * (a + (full * a).sum(-1, keepdim=True)) \
            + abs(g_z) * 2 / T * s.unsqueeze(1) * full
    return dict(idx=idx.to(torch.int32), counts=counts.to(torch.int32),
                aux=aux.detach(), z=z.detach(), z_bound=z_bound,
                dlogits=x.grad, mag=mag)


def assert_aux_close(aux, z, dlogits, ref, what):
    assert aux.dim() == 0 and z.dim() == 0, what
    assert_f32_close(aux.detach().cpu(), ref["aux"], AUX_RTOL, 0.0,
                     what=what + " aux")
    assert_f32_close(z.detach().cpu(), ref["z"], 1.0, 0.0, ref["z_bound"],
                     what + " z")
    assert_bf16_close(dlogits.cpu(), ref["dlogits"], ref["mag"],
                      what + " dlogits")
