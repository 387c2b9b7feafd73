"""The launch sequences of the host layer against a recorded trace.

tests/sanitize/route_trace.cpp walks a fixed table of calls through the C-ABI on the mock HIP runtime
(tests/sanitize/mock_hip.cpp with its trace on).  Every kernel launch (mangled name, grid, block, LDS
bytes, stream, geometry checksum, integer arguments), event record / wait, memset and copy of a call
goes into one line — the number of records and their hash — and after each group the profile's
flops / bytes / launches are printed in full.  The output must equal
tests/golden/route_trace_v1.txt byte for byte: the route rules of csrc/ngp_plan.h and the roofline
formulas of csrc/ngp_cost.h decide nothing else.  To see WHAT moved, run the driver of two builds
with --full (every record in clear) and diff.  The golden file is regenerated only by a change that
means to move a route (build as below, run, write stdout to the file).  No GPU is involved."""
import os
import subprocess

import pytest

from tests.test_host_sanitizers import HIPCC, ROOT, build

GOLDEN = os.path.join(ROOT, "tests", "golden", "route_trace_v1.txt")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_launch_trace_equals_the_recorded_one(tmp_path):
    exe = build(str(tmp_path), [], "plain", "route_trace")
    out = subprocess.run([exe], capture_output=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:].decode() + out.stderr[-2000:].decode()
    with open(GOLDEN, "rb") as f:
        want = f.read()
    got = out.stdout
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        head = next((ln for ln in reversed(g[:k + 1]) if ln.startswith(b"==")), b"")
        pytest.fail(f"trace differs from line {k + 1} ({len(g)} lines against {len(w)}), in {head.decode()} "
                    f"(run the driver with --full for the records):\n"
                    f"  got  {g[k].decode() if k < len(g) else '<end>'}\n"
                    f"  want {w[k].decode() if k < len(w) else '<end>'}")
