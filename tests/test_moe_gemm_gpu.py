"""_hip/moe_gemm.hip on the GPU: expert_mm(impl="hip") forward and backward
per element against fp64 (cases, references and bound in
tests/utils_moe_gemm.py, shown satisfiable in tests/test_moe_gemm_cpu.py),
run-to-run equality, and the composed layer on the hand-written GEMMs."""
import functools

import pytest
import torch

from distributed_training_guide_amd.ops import moe as moe_ops
from utils_moe import MLP_SHAPE, mlp_inputs, mlp_ref64, mlp_run
from utils_moe_gemm import (CASES, assert_gemm_close, gemm_inputs,
                            run_expert_mm)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASES)
def test_expert_mm_hip_matches_fp64_and_repeats(name):
    a, w, dy, offs = gemm_inputs(name, "cuda")
    first = run_expert_mm(moe_ops.expert_mm, a, w, dy, offs)
    assert moe_ops.last_expert_mm_path == "hip"
    assert_gemm_close(name, *first, a, w, dy)
    for x, y in zip(first, run_expert_mm(moe_ops.expert_mm, a, w, dy, offs)):
        assert torch.equal(x, y)


def test_moe_mlp_on_hip_gemms_against_torch_chain():
    """test_moe_mlp_against_torch_chain's criterion with expert_gemm="hip":
    per tensor at most twice the error of moe_mlp_eager on the same device
    against fp64."""
    inp = mlp_inputs("cuda")
    k = MLP_SHAPE["k"]
    ref = mlp_ref64(inp, k, True)
    fused = mlp_run(functools.partial(moe_ops.moe_mlp, expert_gemm="hip"),
                    inp, k, True)
    assert moe_ops.last_expert_mm_path == "hip"
    chain = mlp_run(moe_ops.moe_mlp_eager, inp, k, True)
    for name, f, c, r in zip(("y", "dx", "drouter", "dgate_up", "ddown"),
                             fused, chain, ref):
        ef, ec = (f - r).abs().max().item(), (c - r).abs().max().item()
        print(f"{name}: hip {ef:.4e} chain {ec:.4e}")
        assert ef <= 2.0 * ec, (name, ef, ec)
