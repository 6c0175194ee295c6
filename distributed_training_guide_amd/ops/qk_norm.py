"""QK-norm op: fused qkv split + per-head RMSNorm of q and k + RoPE
(qkv_norm_rope.hip) on GPU, eager fp32 on CPU.

Qwen3, OLMo-2 and Gemma-3 apply an RMSNorm with a learned [head_dim] weight
to every q and k head after the projection and before RoPE.  The kernel that
splits and rotates the packed projection already holds each head row in
registers, so the norm costs one small cross-lane reduction there and no
extra memory traffic in the forward.
"""
import torch

from .._ext import ext, use_hip
from .reference import rope_ref
from .rope import _table_size, get_rope_tables


class _QKVNormRopeFn(torch.autograd.Function):
    """Saves (qkv, wq, wk): the backward recomputes each row's rstd and
    normalised row from the packed projection, which it loads anyway."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, cos, sin, positions, Hq, Hkv, D, eps):
        q, k, v = ext().qkv_norm_rope_fwd(qkv, wq, wk, cos, sin, positions,
                                          Hq, Hkv, D, eps)
        ctx.save_for_backward(qkv, wq, wk)
        ctx.cos, ctx.sin, ctx.positions, ctx.eps = cos, sin, positions, eps
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        qkv, wq, wk = ctx.saved_tensors
        dqkv, dwq, dwk = ext().qkv_norm_rope_bwd(
            dq.contiguous(), dk.contiguous(), dv.contiguous(), qkv, wq, wk,
            ctx.cos, ctx.sin, ctx.positions, ctx.eps)
        return dqkv, dwq, dwk, None, None, None, None, None, None, None


def _head_rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float):
    """rmsnorm_ref's arithmetic on [..., D] head rows, kept in fp32 (no
    rounding between the norm and the rotation, as in the kernel)."""
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return xf * rstd * w.float()


def qkv_norm_rope(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor,
                  Hq: int, Hkv: int, D: int, eps: float,
                  theta: float = 10000.0,
                  positions: torch.Tensor | None = None,
                  max_pos: int | None = None):
    """Split packed qkv [B,S,(Hq+2Hkv)*D], RMS-normalise every q and k head
    row over D with the weights wq / wk [D], then apply RoPE; v is passed
    through.  Returns (q [B,S,Hq,D], k, v [B,S,Hkv,D]).

    Per head row x: y = w * (x * rsqrt(mean(x^2) + eps)), out = rope(y), all
    in fp32 with one rounding to the input dtype at the end (the convention
    of rmsnorm_ref and norm.hip).  HF's Qwen3RMSNorm rounds the normalised
    row to bf16 before multiplying by the weight; this op does not.

    Activation memory: unlike qkv_rope, whose backward needs only the
    tables, this op keeps the packed projection alive until backward
    (W * 2 bytes per token per layer).  Inverting the norm from the output
    would divide by w, so the input is what is kept.

    On the GPU the head dim must be 64 or 128 (the attention kernels accept
    nothing else); any other raises ValueError.  Tables, `positions` and
    `max_pos` follow qkv_rope."""
    B, S, W = qkv.shape
    if use_hip(qkv) and D not in (64, 128):
        raise ValueError(
            f"qkv_norm_rope: head dim {D} is not supported on the GPU "
            "(64 or 128, as the attention kernels)")
    need = _table_size(S, positions, max_pos)
    cos, sin = get_rope_tables(D, need, theta, qkv.device)
    if positions is not None:
        positions = positions.to(torch.int32).contiguous()
    if use_hip(qkv):
        return _QKVNormRopeFn.apply(qkv.contiguous(), wq.contiguous(),
                                    wk.contiguous(), cos, sin, positions,
                                    Hq, Hkv, D, float(eps))
    # CPU: differentiable eager fp32
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q = _head_rmsnorm(q.view(B, S, Hq, D), wq, eps)
    k = _head_rmsnorm(k.view(B, S, Hkv, D), wk, eps)
    q = rope_ref(q, cos, sin, positions).to(qkv.dtype)
    k = rope_ref(k, cos, sin, positions).to(qkv.dtype)
    return q, k, v.view(B, S, Hkv, D).contiguous()
