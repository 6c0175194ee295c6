"""The sorted, atomic-free embedding backward (embedding_bwd_sorted.hip)
against the fp64 scatter sum, and the module's choice of backward."""
import pytest
import torch

from utils_numerics import (assert_bf16_close, embedding_bwd_ref,
                            embedding_inputs)

from distributed_training_guide_amd._ext import ext
from distributed_training_guide_amd.ops.embedding import Embedding

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _edge_ids(ids, V):
    """0, V-1 and pairs that differ only in the top or only in the bottom
    9-bit digit of an 18-bit key, several times each."""
    ids[:4] = 0
    ids[4:8] = V - 1
    ids[8:12] = 5
    ids[12:16] = 5 + 3 * 512
    ids[16:20] = 1025
    ids[20:24] = 1026
    return ids


@pytest.mark.parametrize("V,H,ids_shape,all_equal", [
    (64, 8, (10,), False),          # one active lane, a single sort step
    (3, 50, (7,), False),           # the scalar column path
    (1, 8, (1,), False),            # N = 1, V = 1
    (1024, 520, (8, 512), False),   # second column step, rows never hit
    (16, 8, (33000,), False),       # spans wrap, long rows, the chunk fold
    (16, 8, (33000,), True),        # one row takes everything
    (200000, 8, (5000,), False),    # 18-bit key: two full sort passes
])
def test_sorted_backward_exact(V, H, ids_shape, all_equal):
    _, ids, dy = embedding_inputs(V, H, ids_shape, DEV, all_equal=all_equal)
    if V == 200000:
        ids = _edge_ids(ids, V)
    # every f32 partial sum of this dy is exact in any order: the fp64 sum
    # rounded once is the only correct answer
    dtable = ext().embedding_bwd_sorted(dy, ids, V)
    ref = embedding_bwd_ref(dy, ids, V)
    bad = (dtable != ref).nonzero()
    assert torch.equal(dtable, ref), (
        f"{bad.shape[0]} wrong elements, first at {bad[0].tolist()}: "
        f"{dtable[tuple(bad[0])].item()} vs {ref[tuple(bad[0])].item()}")
    hit = torch.zeros(V, dtype=torch.bool, device=DEV)
    hit[ids.reshape(-1)] = True
    if V >= 1024:
        assert (~hit).any()
    assert torch.equal(dtable[~hit], torch.zeros_like(dtable[~hit]))


@pytest.mark.parametrize("V,H,ids_shape,distinct", [
    (1024, 520, (8, 512), 40),
    (16, 8, (33000,), 16),
])
def test_sorted_backward_order_sensitive(V, H, ids_shape, distinct):
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, distinct, ids_shape, generator=g).to(DEV)
    dy = torch.randn(*ids_shape, H, generator=g).bfloat16().to(DEV)
    flat = dy.reshape(-1, H).double()
    ref = torch.zeros(V, H, dtype=torch.float64, device=DEV)
    ref.index_add_(0, ids.reshape(-1), flat)
    mag = torch.zeros_like(ref).index_add_(0, ids.reshape(-1), flat.abs())
    dtable = ext().embedding_bwd_sorted(dy, ids, V)
    assert_bf16_close(dtable, ref, mag, "sorted dtable")
    assert torch.equal(ext().embedding_bwd_sorted(dy, ids, V), dtable)


@pytest.mark.parametrize("deterministic", [True, False])
def test_module_routes_to_sorted_backward(monkeypatch, deterministic):
    def no_torch(*a, **k):
        raise AssertionError("F.embedding called on the HIP path")

    monkeypatch.setattr(torch.nn.functional, "embedding", no_torch)
    monkeypatch.delenv("DTGA_TORCH_EMBED", raising=False)
    if deterministic:
        monkeypatch.delenv("DTGA_EMBED_BWD", raising=False)
    else:
        monkeypatch.setenv("DTGA_EMBED_BWD", "sorted")
    table, ids, dy = embedding_inputs(40, 104, (4, 64), DEV)
    emb = Embedding(40, 104, device=DEV, dtype=torch.bfloat16)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        with torch.no_grad():
            emb.weight.copy_(table)
        out = emb(ids)
        out.backward(dy)
        assert torch.equal(out, table[ids])
        assert torch.equal(emb.weight.grad,
                           ext().embedding_bwd_sorted(dy, ids, 40))
        if not deterministic:
            monkeypatch.setenv("DTGA_EMBED_BWD", "bogus")
            with pytest.raises(ValueError):
                emb(ids)
    finally:
        torch.use_deterministic_algorithms(was)
