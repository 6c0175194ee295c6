"""Embedding op: HIP gather/scatter-add kernels on GPU (embedding.hip,
embedding_bwd_sorted.hip), F.embedding on CPU — replaces the one torch op
left in the Llama hot loop (SURVEY.md §2b "Embedding gather"; VERDICT round-1 'partial' row)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .._ext import ext, use_hip


class _EmbeddingFn(torch.autograd.Function):
    """sorted_bwd picks the backward: the fp32 atomic scatter-add
    (embedding.hip) or the sorted, atomic-free one with a fixed summation
    order (embedding_bwd_sorted.hip)."""

    @staticmethod
    def forward(ctx, ids, weight, sorted_bwd=False):
        ctx.save_for_backward(ids)
        ctx.V = weight.shape[0]
        ctx.sorted_bwd = sorted_bwd
        return ext().embedding_fwd(weight, ids)

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        if ctx.sorted_bwd:
            dtable = ext().embedding_bwd_sorted(dy.contiguous(), ids, ctx.V)
        else:
            dtable = ext().embedding_bwd(dy.contiguous(), ids, ctx.V)
        return None, dtable, None


class Embedding(nn.Module):
    """Drop-in for nn.Embedding([V, H]) on the gfx950 kernels (fp32
    accumulation in backward, bf16 grad out)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, device=None,
                 dtype=None):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.weight = nn.Parameter(torch.empty(
            num_embeddings, embedding_dim, device=device, dtype=dtype))

    def reset_parameters(self):
        with torch.no_grad():
            if not self.weight.is_meta:
                self.weight.normal_()

    def forward(self, ids):
        import os

        if not use_hip(self.weight) or os.environ.get("DTGA_TORCH_EMBED"):
            return F.embedding(ids, self.weight)
        # the atomic scatter-add's reduction order is run-dependent: the
        # determinism recipe (torch.use_deterministic_algorithms,
        # --deterministic) takes the sorted backward, whose order is a
        # function of ids alone; otherwise DTGA_EMBED_BWD chooses
        if torch.are_deterministic_algorithms_enabled():
            mode = "sorted"
        else:
            mode = os.environ.get("DTGA_EMBED_BWD", "atomic")
            if mode not in ("atomic", "sorted"):
                raise ValueError(
                    f"DTGA_EMBED_BWD must be 'atomic' or 'sorted', got {mode!r}")
        return _EmbeddingFn.apply(ids.contiguous(), self.weight,
                                  mode == "sorted")

    def extra_repr(self):
        return f"{self.num_embeddings}, {self.embedding_dim}"
