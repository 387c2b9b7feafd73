"""The planner of the short-series launch (``small_plan``, csrc/ngp_plan.h) checked on the host
over every geometry it can be asked about (tests/sanitize/plan_check.cpp): what it accepts fits the
kernel's registers, LDS and sweep count and carries every aux row-block exactly once; and ``detect_lattice`` over the date families of
tests/date_cases.py: what it accepts fits its lattice to a measured multiple of eps span; and the
working blocks of a gradient leaf's run (``leaf_run_blocks``) against the two formulas they replaced,
with the rule that sends an item to the Toeplitz leaf (``toep_leaf_item``).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_every_accepted_geometry_fits_the_kernel(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-w",
                           os.path.join(ROOT, "tests", "sanitize", "plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "0 failures" in out.stdout and "1024 geometries accepted" in out.stdout, out.stdout[-500:]
    # the acceptance rule of lattice dates (detect_lattice), swept over n = 2 .. 4096 in the same program
    assert "lattice sweep: 4095 lengths" in out.stdout, out.stdout[-800:]
    # the sizes of a gradient leaf's working blocks: 40 block counts x 3 lengths x 9 lattice settings x
    # 2 paths x invariant on / off x 7 chunk sizes
    assert "leaf blocks: 30240 points" in out.stdout, out.stdout[-800:]
