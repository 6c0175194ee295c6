"""tools/kernel_resources.py: the compiler's per-kernel resource report.

The norm kernels keep their accumulators in registers by design; scratch in
any of them means the compiler moved an array to private memory (a run-time
index into it does that), which no test of results can see.  Needs hipcc,
not a GPU; compiles norm.hip for the device only (a few seconds)."""
import shutil
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))

import kernel_resources  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None,
                                 reason="hipcc not installed")


def test_parse_remarks():
    text = """\
a.hip:27:1: remark: Function Name: _Z3foov [-Rpass-analysis=kernel-resource-usage]
a.hip:27:1: remark:     SGPRs: 30 [-Rpass-analysis=kernel-resource-usage]
a.hip:27:1: remark:     VGPRs: 58 [-Rpass-analysis=kernel-resource-usage]
a.hip:27:1: remark:     ScratchSize [bytes/lane]: 272 [-Rpass-analysis=kernel-resource-usage]
a.hip:27:1: remark:     Occupancy [waves/SIMD]: 8 [-Rpass-analysis=kernel-resource-usage]
a.hip:27:1: remark:     LDS Size [bytes/block]: 32 [-Rpass-analysis=kernel-resource-usage]
"""
    assert kernel_resources.parse_remarks(text) == [
        dict(name="_Z3foov", vgprs=58, scratch=272, occupancy=8, lds=32)]


@needs_hipcc
def test_norm_kernels_use_no_scratch():
    rows = kernel_resources.analyze(kernel_resources.HIP_DIR / "norm.hip")
    names = [r["name"] for r in rows]
    print(*rows, sep="\n")
    # backward per (residual, chunk count) for RMSNorm and per chunk count
    # for LayerNorm; both forwards and the fused forward
    bwd = [n for n in names if "norm_bwd_kernel" in n]
    assert sum(n.startswith("norm_bwd_kernel<false,") for n in bwd) == 8, names
    assert sorted(n for n in bwd if n.startswith("norm_bwd_kernel<true,")) \
        == [f"norm_bwd_kernel<true, false, {c}>" for c in (1, 2, 4)], names
    assert len(bwd) == 11, names
    assert sorted(n for n in names if "norm_fwd_kernel<" in n) == [
        "norm_fwd_kernel<false>", "norm_fwd_kernel<true>"], names
    assert any("add_rmsnorm_fwd_kernel" in n for n in names), names
    for r in rows:
        assert r["scratch"] == 0, r
