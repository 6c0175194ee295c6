"""fp8_delayed.hip in the compiler's resource report: the one-pass cast and
the SwiGLU-to-e4m3 kernel keep a lane's 4x16 patch (and, for SwiGLU, the
sixteen loads that feed it) in registers.  Needs hipcc, not a GPU."""
import shutil
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))

import kernel_resources  # noqa: E402


@pytest.mark.skipif(shutil.which("hipcc") is None,
                    reason="hipcc not installed")
def test_fp8_delayed_kernels_use_no_scratch():
    rows = kernel_resources.analyze(
        kernel_resources.HIP_DIR / "fp8_delayed.hip")
    print(*rows, sep="\n")
    lds = {r["name"]: r["lds"] for r in rows}
    assert lds == {"fp8_cast_amax_kernel<true, true>": 4096,
                   "fp8_cast_amax_kernel<true, false>": 0,
                   "fp8_cast_amax_kernel<false, true>": 4096,
                   "silu_mul_fp8_kernel": 4096,
                   "fp8_history_update_kernel": 64}, lds
    for r in rows:
        assert r["scratch"] == 0, r
