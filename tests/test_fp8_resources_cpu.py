"""fp8_quant.hip in the compiler's resource report (tools/kernel_resources.py).

The cast kernel holds a 4x16 patch of floats per lane in arrays indexed by
compile-time loop variables; a run-time index into one of them would move it
to private memory, which no test of results can see.  Needs hipcc, not a
GPU; compiles fp8_quant.hip for the device only (a few seconds)."""
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
def test_fp8_quant_kernels_use_no_scratch():
    rows = kernel_resources.analyze(kernel_resources.HIP_DIR / "fp8_quant.hip")
    names = sorted(r["name"] for r in rows)
    print(*rows, sep="\n")
    assert names == ["fp8_amax_partials_kernel",
                     "fp8_cast_transpose_kernel<false, true>",
                     "fp8_cast_transpose_kernel<true, false>",
                     "fp8_cast_transpose_kernel<true, true>",
                     "fp8_scale_final_kernel"], names
    for r in rows:
        assert r["scratch"] == 0, r
    lds = {r["name"]: r["lds"] for r in rows}
    # the [64][64] byte image only where a transposed copy is written
    assert lds["fp8_cast_transpose_kernel<true, false>"] == 0
    assert lds["fp8_cast_transpose_kernel<true, true>"] == 4096
    assert lds["fp8_cast_transpose_kernel<false, true>"] == 4096
