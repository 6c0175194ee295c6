"""qkv_norm_rope.hip in the compiler's resource report
(tools/kernel_resources.py).

The backward keeps 32 f32 weight-gradient accumulators per lane across the
whole kernel, next to the row it is working on; arrays indexed at run time
or a register budget that is too small would move them to private memory,
which no test of results can see.  Needs hipcc, not a GPU; compiles
qkv_norm_rope.hip for the device only (a few seconds)."""
import shutil
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))

import kernel_resources  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None,
                                 reason="hipcc not installed")


@needs_hipcc
def test_qkv_norm_rope_kernels_use_no_scratch():
    rows = kernel_resources.analyze(
        kernel_resources.HIP_DIR / "qkv_norm_rope.hip")
    names = sorted(r["name"] for r in rows)
    print(*rows, sep="\n")
    assert names == ["qkv_norm_rope_bwd_kernel<128>",
                     "qkv_norm_rope_bwd_kernel<64>",
                     "qkv_norm_rope_fwd_kernel<128>",
                     "qkv_norm_rope_fwd_kernel<64>"], names
    for r in rows:
        assert r["scratch"] == 0, r
    lds = {r["name"]: r["lds"] for r in rows}
    # the row statistics never go through LDS; the backward's only use is
    # the [4 waves][2*D] f32 image of its final fold
    assert lds["qkv_norm_rope_fwd_kernel<64>"] == 0
    assert lds["qkv_norm_rope_fwd_kernel<128>"] == 0
    assert lds["qkv_norm_rope_bwd_kernel<64>"] == 4 * 2 * 64 * 4
    assert lds["qkv_norm_rope_bwd_kernel<128>"] == 4 * 2 * 128 * 4
