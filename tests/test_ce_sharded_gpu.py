"""Vocab-sharded (loss-parallel) cross entropy: ce_fwd_kernel<true> and
ce_bwd_kernel<true> against the full-vocab fp64 reference, on one GPU with
no process group, plus the public op on a single-rank RCCL group.

A full [B,S,V] logits tensor is split into `tp` contiguous shards; each goes
through ext().ce_fwd_sharded with its vocab_start and the per-row triples
are combined exactly as _ShardedCausalCEFn.forward does across ranks: max,
rescaled sum, max."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import utils_numerics as N
from distributed_training_guide_amd import ops
from distributed_training_guide_amd._ext import ext

DEV = "cuda"
IGN = N.IGNORE_INDEX


def _case(B, S, V, tp, owners):
    g = torch.Generator(device="cpu").manual_seed(31)
    full = torch.randn(B, S, V, generator=g).bfloat16().to(DEV)
    labels = N.ce_sharded_labels(B, S, V, tp, owners).to(DEV)
    Vl = V // tp
    shards = [full[..., r * Vl:(r + 1) * Vl].contiguous() for r in range(tp)]
    return full, labels, shards, Vl


@pytest.mark.parametrize("B,S,V,tp,owners", [
    (2, 9, 96, 3, 3),      # labels on both sides of both boundaries
    (2, 9, 96, 3, 2),      # the last shard owns no label in the batch
    (2, 9, 4160, 2, 2),    # V_local = 2080: the second pass holds one thread
    (3, 700, 64, 2, 2),    # 2097 loss rows > 2048 blocks: row grid-stride
])
def test_sharded_ce_matches_full_vocab(B, S, V, tp, owners):
    full, labels, shards, Vl = _case(B, S, V, tp, owners)
    tgt = labels[:, 1:].reshape(-1)
    valid = tgt != IGN
    for r in range(1, owners):  # both sides of every owning boundary
        assert (tgt == r * Vl - 1).any() and (tgt == r * Vl).any()
    assert (~valid).any()
    ref = N.ce_ref64(full, labels)
    mag = N.ce_row_mag(ref)

    mx, sm, ga = [], [], []
    for r, shard in enumerate(shards):
        m, s, g = ext().ce_fwd_sharded(shard, labels, S - 1, r * Vl, IGN)
        rows = shard[:, :-1].reshape(-1, Vl)
        assert torch.equal(m, rows.float().amax(-1)), f"maxout, shard {r}"
        own = valid & (tgt >= r * Vl) & (tgt < (r + 1) * Vl)
        if r >= owners:
            assert not own.any()
        local = (tgt - r * Vl).clamp(0, Vl - 1)
        want = torch.where(
            own, rows.float().gather(1, local.unsqueeze(1)).squeeze(1),
            torch.full_like(m, -float("inf")))
        assert torch.equal(g, want), f"gathered, shard {r}"
        N.assert_f32_close(s, N.ce_shard_sum_ref64(shard), N.CE_SUM_RTOL,
                           0.0, what=f"sumout, shard {r}")
        mx.append(m), sm.append(s), ga.append(g)

    # the cross-rank combine of _ShardedCausalCEFn.forward
    gmax = torch.stack(mx).amax(0)
    tot = sum(s * torch.exp(m - gmax) for s, m in zip(sm, mx))
    gathered = torch.stack(ga).amax(0)
    lse = gmax + torch.log(tot)
    loss = torch.where(valid, lse - gathered, torch.zeros_like(lse))
    N.assert_f32_close(lse, ref["lse_all"], N.CE_ROW_RTOL, N.CE_ROW_ATOL, mag,
                       "combined lse")
    N.assert_f32_close(loss, ref["loss"], N.CE_ROW_RTOL, N.CE_ROW_ATOL, mag,
                       "combined loss rows")

    # backward: the arithmetic per element is that of the unsharded kernel
    scale = 3.5 / ref["n_valid"]
    parts = [ext().ce_bwd(shard, labels, lse, scale, S - 1, r * Vl, IGN, True)
             for r, shard in enumerate(shards)]
    d = torch.cat(parts, dim=-1)
    whole = ext().ce_bwd(full, labels, lse, scale, S - 1, 0, IGN, False)
    assert torch.equal(d, whole)
    rd, md = N.ce_dlogits_ref64(full, ref, scale)
    N.assert_bf16_close(d, rd, md, "sharded dlogits")
    assert torch.equal(d[:, -1], torch.zeros_like(d[:, -1]))


@pytest.fixture()
def rccl_world1():
    """Single-rank RCCL group, as nccl_world1 in tests/test_rccl_gpu.py, on
    a port of its own."""
    import torch.distributed as dist

    saved = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29547"
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1,
                                device_id=torch.device("cuda:0"))
    yield dist
    if dist.is_initialized():
        dist.destroy_process_group()
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def test_sharded_public_op_single_rank(rccl_world1):
    """ops.sharded_causal_lm_loss on a one-rank group owns the whole vocab:
    loss and logits.grad equal causal_lm_loss on the same tensors, within
    the bounds against fp64."""
    B, S, V = 2, 64, 512
    logits, labels = N.ce_inputs(B, S, V, "normal", DEV)
    ref = N.ce_ref64(logits, labels)
    n = ref["n_valid"]
    want = (ref["loss"].sum() / n).reshape(())
    mean_mag = (N.ce_row_mag(ref).sum() / n).reshape(())

    a = logits.clone().requires_grad_(True)
    la = ops.sharded_causal_lm_loss(a, labels, 0, group=None)
    (la * 3.5).backward()
    b = logits.clone().requires_grad_(True)
    lb = ops.causal_lm_loss(b, labels)
    (lb * 3.5).backward()
    torch.cuda.synchronize()

    # rows within the row bound, the f32 sum of n rows within n * 2^-24
    rtol = N.CE_ROW_RTOL + 2.0 ** -24 * n
    for name, l in (("sharded", la), ("unsharded", lb)):
        N.assert_f32_close(l.detach().reshape(()), want, rtol, N.CE_ROW_ATOL,
                           mean_mag, f"{name} loss")
    rd, md = N.ce_dlogits_ref64(logits, ref, 3.5 / n)
    N.assert_bf16_close(a.grad, rd, md, "sharded grad")
    N.assert_bf16_close(b.grad, rd, md, "unsharded grad")
    assert torch.equal(a.grad[:, -1], torch.zeros_like(a.grad[:, -1]))
