"""_hip/moe_gemm_swiglu.hip on the GPU: the two epilogue-fused kernels per
element against fp64 at the shapes of utils_moe_swiglu.CASES, and the layer
moe_mlp(expert_gemm="hip-fused") against "hip-gather": error, bytes kept for
the backward, run-to-run equality.

The layer's fp64 yardstick is utils_moe.mlp_ref64, which weighs the down
output; in fp64 that is the weighted-SwiGLU layer to 1e-16.  Measured on an
MI355X, max |error| hip-fused / hip-gather: y 1.4958e-02 / 1.4958e-02, dx
3.2096e-02 / 3.2096e-02, drouter 2.0843e-01 / 2.4460e-01, dgate_up
1.5513e-01 / 1.5710e-01, ddown 6.8291e-02 / 8.0818e-02; saved for backward
962288 B / 1095408 B."""
import pytest
import torch

from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops import moe as moe_ops
from test_moe_gemm_gather_gpu import _saved_bytes_and_results
from utils_moe import MLP_SHAPE, mlp_inputs, mlp_ref64
from utils_moe_swiglu import CASES
from utils_numerics import assert_bf16_close, assert_f32_close

pytestmark = pytest.mark.gpu


def _kernels(name):
    idx, E, H, I = CASES[name]
    T, k = idx.shape
    g = torch.Generator().manual_seed(len(name))
    bf = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std) \
        .bfloat16().cuda()  # noqa: E731
    x, gate_up, down = bf(T, H), bf(E, 2 * I, H, std=H ** -0.5), \
        bf(E, H, I, std=I ** -0.5)
    dyp, topk_w = bf(T * k, H), torch.rand(T, k, generator=g).cuda()
    dest, offs = moe_ops.moe_dispatch_index(idx.to(torch.int32).cuda(), E)
    row_src, w_row = moe_ops.moe_row_src(dest, k), \
        moe_ops.moe_row_w(dest, topk_w)
    gu, hw = ext().moe_gemm_gu_swiglu(x, row_src, w_row, gate_up, offs)
    dgu, dw = ext().moe_gemm_da_swiglu(dyp, down, gu, w_row, offs, dest)
    want_gu = moe_ops.expert_mm(x, gate_up, offs, impl="hip-gather",
                                row_src=row_src, dest=dest)
    return (gu, hw, dgu, dw), want_gu, (dyp, down, w_row, topk_w, dest, offs)


@pytest.mark.parametrize("name", CASES)
def test_kernels_against_fp64_and_repeat(name):
    (gu, hw, dgu, dw), want_gu, (dyp, down, w_row, topk_w, dest, offs) = \
        _kernels(name)
    for a, b in zip((gu, hw, dgu, dw), _kernels(name)[0]):
        assert torch.equal(a, b), name
    assert torch.equal(w_row[dest.long()], topk_w.reshape(-1))
    assert torch.equal(gu, want_gu)

    H, I = down.shape[1:]
    g, u = gu[:, :I].double().cpu(), gu[:, I:].double().cpu()
    w = w_row.double().cpu().unsqueeze(1)
    sig = torch.sigmoid(g)
    s = g * sig * u
    assert_bf16_close(hw.cpu(), w * s, what=f"{name} h'")

    # dh' = dyp . down[e] in fp64 with the magnitude of its terms.  The
    # kernel's f32 dh' is within 2^-16 f mag of it, f as in
    # utils_moe_gemm.assert_gemm_close for a contraction of H; that error is
    # carried through w and the derivative factors' magnitudes (the bracket
    # 1 + g (1 - sig) cancels for g < 0, as in silu_mul_bwd_ref64), and the
    # f32 evaluation of those factors adds 2^-16 of |dh'| <= mag times them:
    # (f + 1) w mag D under assert_bf16_close's 2^-16.
    d64, wd = dyp.double().cpu(), down.double().cpu()
    dh, mag, lo = torch.empty_like(g), torch.empty_like(g), 0
    for e, hi in enumerate(offs.tolist()):
        dh[lo:hi] = d64[lo:hi] @ wd[e]
        mag[lo:hi] = d64[lo:hi].abs() @ wd[e].abs()
        lo = hi
    f = max(1.0, (H + 1) / 256)
    t = g * (1 - sig)
    ref = torch.cat([w * dh * u * sig * (1 + t), w * dh * g * sig], 1)
    dmag = torch.cat([(u * sig).abs() * (1 + t.abs()), (g * sig).abs()], 1)
    assert_bf16_close(dgu.cpu(), ref, (f + 1) * w * mag.repeat(1, 2) * dmag,
                      f"{name} dgu")
    # dw: the same error of dh' and of s on every term, plus an I-term f32
    # row sum in any order, max(1, (I + 1) / 256) of the terms' magnitudes
    rmag = (f + 1) * (mag * s.abs()).sum(1) \
        + max(1.0, (I + 1) / 256) * (dh * s).abs().sum(1)
    sel = dest.long().cpu()
    assert_f32_close(dw.cpu(), (dh * s).sum(1)[sel], 2.0 ** -16, 0.0,
                     rmag[sel], f"{name} dw_topk")


def test_layer_error_saved_bytes_and_repeat():
    inp, s = mlp_inputs("cuda"), MLP_SHAPE
    ref = mlp_ref64(inp, s["k"], True)
    gather_bytes, gather = _saved_bytes_and_results("hip-gather", inp, s["k"])
    fused_bytes, fused = _saved_bytes_and_results("hip-fused", inp, s["k"])
    assert moe_ops.last_expert_mm_path == "hip-fused"
    for a, b in zip(fused,
                    _saved_bytes_and_results("hip-fused", inp, s["k"])[1]):
        assert torch.equal(a, b)
    print(f"saved for backward: hip-gather {gather_bytes} B, "
          f"hip-fused {fused_bytes} B")
    slots = s["T"] * s["k"]
    assert fused_bytes <= gather_bytes - slots * s["H"] * 2 + 8 * slots
    # no more than twice the existing path's own error: one more rounding,
    # of w * h
    for name, a, b, r in zip(("y", "dx", "drouter", "dgate_up", "ddown"),
                             fused, gather, ref):
        ef, eg = (a - r).abs().max().item(), (b - r).abs().max().item()
        print(f"{name}: hip-fused {ef:.4e} hip-gather {eg:.4e}")
        assert ef <= 2.0 * eg, (name, ef, eg)
