"""Cases, inputs, fp64 references and the bound shared by
tests/test_moe_gemm_cpu.py and tests/test_moe_gemm_gpu.py."""
import torch

from utils_numerics import assert_bf16_close

# name -> (rows per expert, K, M): the smallest shapes at which the tile
# search, the ragged masking, the double buffer and the column remainder of
# _hip/moe_gemm.hip can each go wrong
CASES = {
    # empty groups first and in the middle, one row, both sides of a 64-row
    # boundary, more than one tile, a single K-step
    "ragged": ((0, 1, 63, 64, 65, 0, 257, 130), 64, 64),
    # every row on the last expert, an odd number of K-steps, columns a
    # multiple of 64 but not of 128
    "last_only": ((0, 0, 0, 0, 0, 0, 0, 200), 192, 320),
    # a dW walk of many steps with a ragged tail, E not a power of two
    "long_group": ((3, 1100, 0, 45), 256, 128),
    # E = 128, far more tiles than full tiles, many empty experts
    "many_small": (tuple(torch.randint(
        0, 4, (128,), generator=torch.Generator().manual_seed(1)).tolist()),
        128, 192),
}


def gemm_inputs(name, device):
    """(a [N, K], weight [E, M, K], dy [N, M], offs int32 [E]), bf16."""
    rows, K, M = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    N, E = sum(rows), len(rows)
    a = torch.randn(N, K, generator=g).bfloat16()
    w = (torch.randn(E, M, K, generator=g) * K ** -0.5).bfloat16()
    dy = torch.randn(N, M, generator=g).bfloat16()
    offs = torch.tensor(rows).cumsum(0).to(torch.int32)
    return a.to(device), w.to(device), dy.to(device), offs.to(device)


def assert_gemm_close(name, y, da, dw, a, w, dy):
    """y, da and every dw[e] against the per-expert fp64 products of the
    same bf16 inputs: one bf16 rounding plus an L-term f32 dot product in
    any order, mag * max(1, (L + 1) / 256) under assert_bf16_close's 2^-16,
    L the contraction length.  An empty expert's dw is exactly zero."""
    rows, K, M = CASES[name]
    a64, w64, d64 = a.double().cpu(), w.double().cpu(), dy.double().cpu()
    y, da, dw = y.cpu(), da.cpu(), dw.cpu()
    lo = 0
    for e, n in enumerate(rows):
        A, D, W, hi = a64[lo:lo + n], d64[lo:lo + n], w64[e], lo + n
        for out, ref, mag, L, what in (
                (y[lo:hi], A @ W.T, A.abs() @ W.abs().T, K, "y"),
                (da[lo:hi], D @ W, D.abs() @ W.abs(), M, "da"),
                (dw[e], D.T @ A, D.abs().T @ A.abs(), n, "dw")):
            assert_bf16_close(out, ref, mag * max(1.0, (L + 1) / 256),
                              f"{name} {what} expert {e}")
        if n == 0:
            assert bool((dw[e] == 0).all()), f"{name} dw of empty expert {e}"
        lo = hi


def run_expert_mm(expert_mm, a, w, dy, offs, impl="hip"):
    """(y, da, dw) of expert_mm under the upstream gradient dy."""
    a, w = a.clone().requires_grad_(), w.clone().requires_grad_()
    y = expert_mm(a, w, offs, impl=impl)
    y.backward(dy)
    return y.detach(), a.grad, w.grad
