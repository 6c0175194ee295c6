"""Causal flash attention op (BSHD layout, GQA).

HIP MFMA kernels on GPU (attention_fwd.hip / attention_bwd.hip) — the
replacement for the reference's flash-attn-2 dependency
(attn_implementation="flash_attention_2",
/root/reference/05-training-llama-405b/train_llm.py:87-94).  CPU path uses
torch SDPA in fp32 (differentiable, reference numerics).

With `doc` (ops/doc_mask.py) attention is additionally confined to each
token's own document of a packed row — flash-attn-2's varlen masking.
"""
import math

import torch

from .._ext import ext, use_hip
from .doc_mask import DocBounds, as_doc_bounds
from .reference import attention_ref


class _FlashAttnFn(torch.autograd.Function):
    """doc_start / doc_end: the int32 [B,S] tables of a DocBounds, or both
    None for plain causal attention."""

    @staticmethod
    def forward(ctx, q, k, v, doc_start, doc_end, scale):
        if doc_start is None:
            o, lse = ext().attn_fwd(q, k, v, scale)
            ctx.save_for_backward(q, k, v, o, lse)
        else:
            o, lse = ext().attn_fwd_doc(q, k, v, doc_start, scale)
            ctx.save_for_backward(q, k, v, o, lse, doc_start, doc_end)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, *doc = ctx.saved_tensors
        bwd = ext().attn_bwd_doc if doc else ext().attn_bwd
        dq, dk, dv = bwd(dout.contiguous(), q, k, v, o, lse, *doc, ctx.scale)
        return dq, dk, dv, None, None, None


def _check_doc(doc: DocBounds, q: torch.Tensor) -> None:
    for name, t in (("doc.start", doc.start), ("doc.end", doc.end)):
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, got {t.dtype}")
        if t.shape != q.shape[:2]:
            raise ValueError(f"{name} must be [B,S] = {tuple(q.shape[:2])}, "
                             f"got {tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name} must be on q's device {q.device}, "
                             f"got {t.device}")


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    scale: float | None = None, doc=None) -> torch.Tensor:
    """q [B,S,Hq,D], k/v [B,S,Hkv,D] -> o [B,S,Hq,D]; always causal.

    doc: a DocBounds or a raw doc_start tensor (int32 [B,S] on q's device);
    query i then sees key j iff doc_start[b,i] <= j <= i.  Pass a DocBounds
    when several layers share one mask — a raw tensor derives the second
    table on every call."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    start = end = None
    if doc is not None:
        doc = as_doc_bounds(doc)
        _check_doc(doc, q)
        start, end = doc.start.contiguous(), doc.end.contiguous()
    if use_hip(q, k, v):
        return _FlashAttnFn.apply(q.contiguous(), k.contiguous(),
                                  v.contiguous(), start, end, scale)
    return attention_ref(q, k, v, scale, start)
