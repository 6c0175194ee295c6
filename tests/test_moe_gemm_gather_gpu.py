"""_hip/moe_gemm_gather.hip on the GPU: expert_mm(impl="hip-gather") reads
the unsorted tokens through moe_row_src's index.  Forward, dx and dw equal
the bits of impl="hip" on the scattered copy (same arithmetic, same order),
stay per element inside the fp64 bound of tests/utils_moe_gemm.py, and the
composed layer keeps one [T*k, H] tensor less for its backward."""
import functools

import pytest
import torch

import utils_moe_gemm
from distributed_training_guide_amd.ops import moe as moe_ops
from utils_moe import MLP_SHAPE, mlp_inputs, mlp_run
from utils_numerics import assert_bf16_close

pytestmark = pytest.mark.gpu


def _pick(T, k, allowed, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(allowed)[torch.randint(len(allowed), (T, k),
                                               generator=g)]


# name -> (topk_idx [T, k], E, K, M)
GATHER_CASES = {
    # experts 0 and 5 never chosen (empty groups first and in the middle),
    # 520 rows on six experts (ragged tiles), a single K-step
    "ragged": (_pick(65, 8, (1, 2, 3, 4, 6, 7), 1), 8, 64, 64),
    # many tiny groups, columns a multiple of 64 but not of 128
    "many_small": (_pick(40, 3, tuple(range(128)), 2), 128, 128, 192),
    # one 1100-row group: the dW walk's two-ahead index pipeline wraps 17
    # times and ends in a ragged step of 12 rows
    "one_expert": (torch.full((1100, 1), 2), 4, 256, 128),
    "single": (torch.full((1, 1), 3), 8, 64, 64),
}


def _inputs(name):
    idx, E, K, M = GATHER_CASES[name]
    T, k = idx.shape
    g = torch.Generator().manual_seed(len(name))
    x = torch.randn(T, K, generator=g).bfloat16().cuda()
    w = (torch.randn(E, M, K, generator=g) * K ** -0.5).bfloat16().cuda()
    dy = torch.randn(T * k, M, generator=g).bfloat16().cuda()
    # the index build takes E >= 8; experts past E get no slot, so the first
    # E offsets are the table of E experts
    dest, offs = moe_ops.moe_dispatch_index(idx.to(torch.int32).cuda(),
                                            max(E, 8))
    return x, w, dy, dest, offs[:E].contiguous(), k


@pytest.mark.parametrize("name", GATHER_CASES)
def test_gather_equals_scattered_hip_and_fp64(name, monkeypatch):
    x, w, dy, dest, offs, k = _inputs(name)
    T, N = x.shape[0], dest.numel()
    row_src = moe_ops.moe_row_src(dest, k)
    inv = torch.empty(N, dtype=torch.long, device="cuda")
    inv[dest.long()] = torch.arange(N, device="cuda") // k
    assert row_src.dtype == torch.int32 and torch.equal(row_src.long(), inv)

    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = moe_ops.expert_mm(xg, wg, offs, impl="hip-gather", row_src=row_src,
                          dest=dest)
    assert moe_ops.last_expert_mm_path == "hip-gather"
    y.backward(dy)

    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    xp = moe_ops.moe_scatter(xs, dest, k)
    xp.retain_grad()
    ys = moe_ops.expert_mm(xp, ws, offs, impl="hip")
    ys.backward(dy)
    assert torch.equal(y, ys)
    assert torch.equal(xg.grad, xs.grad)
    assert torch.equal(wg.grad, ws.grad)

    # y and dw per element against fp64 (the sorted da is the scattered
    # path's: the gather path only ever returns its k-way sum)
    rows = torch.diff(offs.cpu(), prepend=torch.zeros(1, dtype=torch.int32))
    _, E, K, M = GATHER_CASES[name]
    monkeypatch.setitem(utils_moe_gemm.CASES, name, (tuple(rows.tolist()), K, M))
    utils_moe_gemm.assert_gemm_close(name, y.detach(), xp.grad, wg.grad,
                                     xp.detach(), w, dy)
    # dx[t] = sum_j dxp[dest[t*k + j]] in fp64.  Every sorted row is rounded
    # to bf16 (2^-8 |dxp|) on top of its GEMM error (2^-16 f mag, f as in
    # assert_gemm_close), the k <= 8 f32 adds cost at most 8 * 2^-24 of the
    # terms' magnitudes, and the final rounding, which assert_bf16_close
    # allows on |ref|, also carries those errors (a factor 1 + 2^-8): in
    # units of 2^-16, (2^8 + 2) |dxp| + 2 f mag per term.
    d64, w64 = dy.double().cpu(), w.double().cpu()
    dxp, mag, lo = torch.empty(N, K).double(), torch.empty(N, K).double(), 0
    for e, n in enumerate(rows.tolist()):
        dxp[lo:lo + n] = d64[lo:lo + n] @ w64[e]
        mag[lo:lo + n] = d64[lo:lo + n].abs() @ w64[e].abs()
        lo += n
    f = max(1.0, (M + 1) / 256)
    sel = dest.long().cpu().view(T, k)
    assert_bf16_close(xg.grad.cpu(), dxp[sel].sum(1),
                      (258.0 * dxp.abs() + 2.0 * f * mag)[sel].sum(1),
                      f"{name} dx")


def _saved_bytes_and_results(expert_gemm, inp, k):
    """mlp_run's results and the bytes the forward keeps for the backward:
    every saved tensor's storage, counted once."""
    kept = {}

    def pack(t):
        s = t.untyped_storage()
        kept[s.data_ptr()] = s.nbytes()
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = mlp_run(functools.partial(moe_ops.moe_mlp,
                                        expert_gemm=expert_gemm), inp, k, True)
    return sum(kept.values()), out


def test_moe_mlp_gather_keeps_no_scattered_copy():
    inp = mlp_inputs("cuda")
    s = MLP_SHAPE
    hip_bytes, hip = _saved_bytes_and_results("hip", inp, s["k"])
    gather_bytes, gather = _saved_bytes_and_results("hip-gather", inp, s["k"])
    print(f"saved for backward: hip {hip_bytes} B, hip-gather {gather_bytes} B")
    assert hip_bytes - gather_bytes >= s["T"] * s["k"] * s["H"] * 2
    for name, a, b in zip(("y", "dx", "drouter", "dgate_up", "ddown"),
                          gather, hip):
        assert torch.equal(a, b), name
