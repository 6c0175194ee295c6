"""Document tables for masked causal attention over packed rows.

data/pipeline.py packs documents into one flat stream with an EOS
separator; plain causal attention then lets a token attend to unrelated
earlier documents of its row.  The doc-masked attention mode
(flash_attention(..., doc=...)) restricts query i to the keys of its own
document, described by one int32 table:

    doc_start[b, i] = index of the first token of the document holding i

Contract: 0 <= doc_start[b,i] <= i; non-decreasing along i;
doc_start[b, doc_start[b,i]] == doc_start[b,i].  Query i sees key j iff
doc_start[b,i] <= j <= i.  An EOS token belongs to the document it ends;
the next document starts at the token after it, and every row starts a
document at index 0.

The derived table doc_end[b, j] is the exclusive end of j's document (S for
the last one).  The kernels read whichever table is lane-local in their
fragment layout: forward and dq own q rows (doc_start), dk/dv owns keys
(doc_end).
"""
from typing import NamedTuple

import torch


class DocBounds(NamedTuple):
    """Both tables, int32 [B,S] contiguous.  Build once per model forward
    (doc_bounds) and hand the same object to every attention layer."""
    start: torch.Tensor
    end: torch.Tensor


def doc_start_from_ids(input_ids: torch.Tensor, eos_id: int) -> torch.Tensor:
    """[B,S] token ids -> doc_start int32 [B,S].  Pure tensor ops, no host
    sync; works on CPU and GPU."""
    if input_ids.dim() != 2:
        raise ValueError("input_ids must be [B,S]")
    S = input_ids.shape[1]
    idx = torch.arange(S, device=input_ids.device, dtype=torch.int32)
    # a document starts at 0 and after every EOS
    is_start = torch.ones_like(input_ids, dtype=torch.bool)
    is_start[:, 1:] = input_ids[:, :-1] == eos_id
    marks = torch.where(is_start, idx, torch.zeros_like(idx))
    return torch.cummax(marks, dim=1).values.contiguous()


def doc_bounds(doc_start: torch.Tensor) -> DocBounds:
    """doc_start [B,S] -> DocBounds(start, end), on doc_start's device with
    no host sync."""
    if doc_start.dim() != 2:
        raise ValueError("doc_start must be [B,S]")
    if doc_start.dtype != torch.int32:
        raise ValueError("doc_start must be int32")
    start = doc_start.contiguous()
    B, S = start.shape
    idx = torch.arange(S, device=start.device, dtype=torch.int32)
    # exclusive end of j's document = the next document start after j:
    # a reversed running minimum over the start positions (S where none)
    is_start = start == idx
    nxt = torch.where(is_start, idx, torch.full_like(idx, S)).expand(B, S)
    nxt = torch.cat([nxt[:, 1:], nxt.new_full((B, 1), S)], dim=1)
    end = torch.cummin(nxt.flip(1), dim=1).values.flip(1).contiguous()
    return DocBounds(start, end)


def as_doc_bounds(doc) -> DocBounds:
    """Accept a DocBounds or a raw doc_start tensor."""
    if isinstance(doc, DocBounds):
        return doc
    if isinstance(doc, torch.Tensor):
        return doc_bounds(doc)
    raise ValueError("doc must be a DocBounds or a doc_start tensor")


def validate_doc_start(doc_start: torch.Tensor) -> None:
    """Debug-only check of the doc_start contract (raises ValueError).
    Syncs with the host — never call it on the hot path."""
    if doc_start.dim() != 2 or doc_start.dtype != torch.int32:
        raise ValueError("doc_start must be int32 [B,S]")
    S = doc_start.shape[1]
    ds = doc_start.long()
    idx = torch.arange(S, device=ds.device)
    if bool(((ds < 0) | (ds > idx)).any()):
        raise ValueError("doc_start[b,i] must lie in [0, i]")
    if bool((ds[:, 1:] < ds[:, :-1]).any()):
        raise ValueError("doc_start must be non-decreasing along the row")
    if not torch.equal(torch.gather(ds, 1, ds), ds):
        raise ValueError("doc_start[b, doc_start[b,i]] must equal "
                         "doc_start[b,i]")
