"""expert_gemm="hip-gather" without a GPU: on CPU tensors it is the eager
chain (scatter, then the torch GEMM), and the kernels of
_hip/moe_gemm_gather.hip compile to 0 bytes of scratch."""
import shutil

import pytest
import torch

from distributed_training_guide_amd.ops import moe as moe_ops
from utils_moe import MLP_SHAPE, mlp_inputs, mlp_run


def test_hip_gather_on_cpu_is_the_eager_chain():
    inp, k = mlp_inputs("cpu"), MLP_SHAPE["k"]
    gather = mlp_run(lambda *a: moe_ops.moe_mlp(*a, expert_gemm="hip-gather"),
                     inp, k, True)
    for a, b in zip(gather, mlp_run(moe_ops.moe_mlp_eager, inp, k, True)):
        assert torch.equal(a, b)


def test_expert_mm_row_src_on_cpu_scatters_first():
    g = torch.Generator().manual_seed(3)
    T, k, E, K, M = 9, 2, 4, 64, 128
    idx = torch.randint(0, E, (T, k), generator=g)
    dest, offs = moe_ops.moe_dispatch_index(idx, E)
    row_src = moe_ops.moe_row_src(dest, k)
    assert row_src.dtype == torch.int32
    assert torch.equal(row_src[dest.long()].long(),
                       torch.arange(T * k) // k)
    x = torch.randn(T, K, generator=g).bfloat16()
    w = torch.randn(E, M, K, generator=g).bfloat16()
    want = moe_ops.expert_mm(moe_ops.moe_scatter(x, dest, k), w, offs)
    got = moe_ops.expert_mm(x, w, offs, impl="hip-gather", row_src=row_src,
                            dest=dest)
    assert moe_ops.last_expert_mm_path in ("grouped", "loop")
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="row_src"):
        moe_ops.expert_mm(x, w, offs, impl="hip-gather", row_src=row_src)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_gather_kernels_use_no_scratch():
    from test_kernel_resources_cpu import kernel_resources
    rows = kernel_resources.analyze(
        kernel_resources.HIP_DIR / "moe_gemm_gather.hip")
    assert len(rows) == 3, rows
    for r in rows:
        assert r["scratch"] == 0, r
