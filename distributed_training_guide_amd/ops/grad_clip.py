"""Global gradient-norm clipping on the gfx950 HIP kernels (grad_norm.hip).

`grad_sq_sum` is one read-only multi-tensor pass over the grads (same
chunk-descriptor table as FusedAdamW); the result stays on the device.
`clip_grad_norm_` is the drop-in for any optimizer: norm, then an in-place
multi-tensor scale whose coefficient is computed in-kernel from the device
scalar.  Nothing here calls `.item()`/`.cpu()` or synchronizes.  FusedAdamW
fuses the scale into its update instead (`max_grad_norm=`), so the grads are
never rewritten.

Sharded engines see only part of the gradient on each rank, so both entry
points take `parts`: a list of `(params, process_group_or_None)`.  Each
part's local squared sum is all-reduced (SUM) over its group when the group
is not None, then the parts are added:

  single / DDP / ZeRO-1   [(all params, None)]       grads complete per rank
  FSDP                    [(flat shards, fsdp group)]
  TP                      [(sharded, tp group), (replicated norms, None)]

CPU path (cpu-offload, unit tests): eager fp32 math, same formula.
"""
import torch
import torch.distributed as dist

from .._ext import ext, use_hip
from .adamw import CHUNK

EPS = 1e-6  # torch.nn.utils.clip_grad_norm_'s denominator epsilon


def _as_list(tensors_or_params):
    if isinstance(tensors_or_params, torch.Tensor):
        return [tensors_or_params]
    return list(tensors_or_params)


def _grads(tensors_or_params):
    return [t.grad for t in _as_list(tensors_or_params)
            if t.grad is not None]


class _GradTable:
    """Chunk-descriptor tables over a list of grads, cached and rebuilt only
    when the grad addresses change (keyed on (data_ptr, numel) like
    FusedAdamW._step_hip).  A few entries are kept: the autograd allocator
    cycles through a small set of addresses under zero_grad(set_to_none)."""

    MAX_ENTRIES = 8

    def __init__(self):
        self._cache = {}

    def get(self, grads):
        key = tuple((g.data_ptr(), g.numel(), g.dtype) for g in grads)
        hit = self._cache.get(key)
        if hit is not None:
            return hit
        import numpy as np

        blocks = []
        for g in grads:
            if not g.is_contiguous():
                raise RuntimeError("grad clipping requires contiguous grads")
            if g.dtype not in (torch.bfloat16, torch.float32):
                raise RuntimeError(f"unsupported grad dtype {g.dtype}")
            if g.device != grads[0].device:
                raise RuntimeError("grads of one part must share a device")
            g_bf = 1 if g.dtype == torch.bfloat16 else 0
            n = g.numel()
            offs = np.arange(0, n, CHUNK, dtype=np.int64)
            rows = np.zeros((len(offs), 7), dtype=np.int64)
            rows[:, 1] = g.data_ptr() + offs * (2 if g_bf else 4)
            rows[:, 4] = np.minimum(CHUNK, n - offs)
            rows[:, 6] = g_bf
            blocks.append(rows)
        table = np.concatenate(blocks) if blocks \
            else np.zeros((0, 7), dtype=np.int64)
        dev = grads[0].device
        desc = torch.from_numpy(table).to(dev, non_blocking=True)
        partials = torch.empty(max(len(table), 1), dtype=torch.float32,
                               device=dev)
        if len(self._cache) >= self.MAX_ENTRIES:
            self._cache.pop(next(iter(self._cache)))
        self._cache[key] = (desc, len(table), partials)
        return self._cache[key]


_TABLES = _GradTable()


def _local_sq_sum(grads, tables):
    """0-dim fp32 squared L2 sum of `grads` (non-empty) on their device."""
    if use_hip(*grads):
        desc, nchunks, partials = tables.get(grads)
        out = torch.empty(1, dtype=torch.float32, device=grads[0].device)
        ext().grad_sqsum(desc, nchunks, partials, out, 0)
        return out[0]
    total = grads[0].float().pow(2).sum()
    for g in grads[1:]:
        total = total + g.float().pow(2).sum()
    return total


def _all_reduce_sum(t, group):
    if dist.get_backend(group) == "nccl" and not t.is_cuda:
        # cpu-offloaded shards under an RCCL group: reduce on the device
        dev = torch.device("cuda", torch.cuda.current_device())
        t = t.to(dev)
        dist.all_reduce(t, group=group)
        return t.cpu()
    t = t.reshape(1)
    dist.all_reduce(t, group=group)
    return t[0]


def total_sq_sum(parts, tables=None):
    """Global squared grad norm over `parts` (see the module docstring);
    0-dim fp32 on the grads' device.  Every rank of a part's group must
    call this, also a rank whose local grads are all None."""
    tables = tables or _TABLES
    total = None
    for params, group in parts:
        grads = _grads(params)
        if grads:
            sq = _local_sq_sum(grads, tables)
        elif group is None:
            continue
        else:
            sq = torch.zeros((), dtype=torch.float32)
        if group is not None:
            sq = _all_reduce_sum(sq, group)
        total = sq if total is None else total + sq.to(total.device)
    if total is None:
        total = torch.zeros((), dtype=torch.float32)
    return total


def grad_sq_sum(tensors_or_params):
    """Squared L2 sum of all `.grad`s (None skipped) as a 0-dim fp32 tensor
    on the grads' device."""
    return total_sq_sum([(_as_list(tensors_or_params), None)])


def clip_coef(total_sq, max_norm):
    """Eager form of the kernels' scale: max_norm / (norm + 1e-6), clamped
    to 1 (a NaN norm stays NaN, as with torch.clamp)."""
    return (max_norm / (total_sq.sqrt() + EPS)).clamp(max=1.0)


@torch.no_grad()
def clip_grad_norm_(params, max_norm, parts=None):
    """Scale the grads of `params` in place so that the global norm (over
    `parts`, default: `params` itself, complete on this rank) is at most
    `max_norm`.  Returns the pre-clip total norm, a 0-dim fp32 tensor."""
    params = _as_list(params)
    if parts is None:
        parts = [(params, None)]
    else:
        parts = [(_as_list(ps), group) for ps, group in parts]
    total_sq = total_sq_sum(parts)
    grads = _grads(params)
    if grads:
        if use_hip(*grads):
            desc, nchunks, _ = _TABLES.get(grads)
            ext().grad_scale_(desc, nchunks,
                              total_sq.to(grads[0].device).reshape(1),
                              float(max_norm))
        else:
            coef = clip_coef(total_sq, float(max_norm))
            for g in grads:
                g.mul_(coef.to(g.device))
    return total_sq.sqrt()
