"""expert_mm's `impl` argument on the CPU: impl="hip" on CPU tensors takes
the torch path, which shows that the references and the bound of
tests/utils_moe_gemm.py are satisfiable; the argument check; the config
field reaching moe_mlp; and the new kernels' scratch."""
import dataclasses
import shutil

import pytest
import torch

from distributed_training_guide_amd.models import build_model, get_config
from distributed_training_guide_amd.models import llama
from distributed_training_guide_amd.ops import moe as moe_ops
from utils_moe_gemm import (CASES, assert_gemm_close, gemm_inputs,
                            run_expert_mm)


@pytest.mark.parametrize("name", CASES)
def test_torch_path_is_inside_the_bound(name):
    a, w, dy, offs = gemm_inputs(name, "cpu")
    out = run_expert_mm(moe_ops.expert_mm, a, w, dy, offs, impl="hip")
    assert moe_ops.last_expert_mm_path in ("grouped", "loop")
    assert_gemm_close(name, *out, a, w, dy)


def test_unknown_impl_is_rejected():
    a, w, _, offs = gemm_inputs("ragged", "cpu")
    with pytest.raises(ValueError, match="impl"):
        moe_ops.expert_mm(a, w, offs, impl="bogus")
    with pytest.raises(ValueError, match="expert_gemm"):
        moe_ops.moe_mlp(a, w[:, 0], w, w, 2, expert_gemm="bogus")


@pytest.mark.parametrize("impl", ["torch", "hip"])
def test_config_reaches_moe_mlp(impl, monkeypatch):
    seen = []

    def spy(*args, expert_gemm="torch", **kw):
        seen.append(expert_gemm)
        return moe_ops.moe_mlp(*args, expert_gemm=expert_gemm, **kw)

    monkeypatch.setattr(llama, "moe_mlp", spy)
    cfg = dataclasses.replace(get_config("qwen3-moe-debug"), expert_gemm=impl)
    ids = torch.randint(0, cfg.vocab_size, (1, 16))
    build_model(cfg)(input_ids=ids)
    assert seen == [impl] * cfg.num_hidden_layers


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_moe_gemm_kernels_use_no_scratch():
    from test_kernel_resources_cpu import kernel_resources
    rows = kernel_resources.analyze(kernel_resources.HIP_DIR / "moe_gemm.hip")
    assert len(rows) == 3, rows
    for r in rows:
        assert r["scratch"] == 0, r
