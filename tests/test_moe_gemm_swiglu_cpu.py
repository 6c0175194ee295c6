"""expert_gemm="hip-fused" without a GPU: on CPU tensors the layer and
expert_mm are the torch path, the config field and the trainer's flag take
the value, and the kernels of _hip/moe_gemm_swiglu.hip compile to 0 bytes of
scratch."""
import dataclasses
import shutil

import pytest
import torch

from distributed_training_guide_amd.models import build_model, get_config
from distributed_training_guide_amd.ops import moe as moe_ops
from distributed_training_guide_amd.trainer import get_parser
from utils_moe import MLP_SHAPE, mlp_inputs, mlp_run
from utils_moe_swiglu import CASES


def test_hip_fused_on_cpu_is_the_torch_layer():
    inp, k = mlp_inputs("cpu"), MLP_SHAPE["k"]
    fused = mlp_run(lambda *a: moe_ops.moe_mlp(*a, expert_gemm="hip-fused"),
                    inp, k, True)
    for a, b in zip(fused, mlp_run(moe_ops.moe_mlp, inp, k, True)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_expert_mm_hip_fused_on_cpu_is_torch(name):
    idx, E, H, I = CASES[name]
    T, k = idx.shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, H, generator=g).bfloat16()
    w = torch.randn(E, 2 * I, H, generator=g).bfloat16()
    dest, offs = moe_ops.moe_dispatch_index(idx, E)
    assert torch.equal(torch.diff(offs, prepend=offs.new_zeros(1)),
                       torch.bincount(idx.reshape(-1), minlength=E))
    want = moe_ops.expert_mm(moe_ops.moe_scatter(x, dest, k), w, offs)
    got = moe_ops.expert_mm(x, w, offs, impl="hip-fused",
                            row_src=moe_ops.moe_row_src(dest, k), dest=dest)
    assert torch.equal(got, want)
    assert torch.equal(
        moe_ops.expert_mm(moe_ops.moe_scatter(x, dest, k), w, offs,
                          impl="hip-fused"), want)
    topk_w = torch.rand(T, k, generator=g)
    assert torch.equal(moe_ops.moe_row_w(dest, topk_w)[dest.long()],
                       topk_w.reshape(-1))


def test_config_and_cli_take_hip_fused():
    assert "hip-fused" in moe_ops.EXPERT_GEMM_IMPLS
    cfg = dataclasses.replace(get_config("qwen3-moe-debug"),
                              expert_gemm="hip-fused")
    ids = torch.randint(0, cfg.vocab_size, (1, 16))
    assert build_model(cfg)(input_ids=ids).logits.shape[:2] == (1, 16)
    args = get_parser().parse_args(["-m", "qwen3-moe-debug", "--expert-gemm",
                                    "hip-fused"])
    assert args.expert_gemm == "hip-fused"


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_swiglu_gemm_kernels_use_no_scratch():
    from test_kernel_resources_cpu import kernel_resources
    rows = kernel_resources.analyze(
        kernel_resources.HIP_DIR / "moe_gemm_swiglu.hip")
    assert len(rows) == 4, rows
    for r in rows:
        assert r["scratch"] == 0, r
