"""The copies and launches of the one-shot device calls against a recorded trace.

tests/sanitize/oneshot_trace.cpp walks the table of tests/sanitize/oneshot_calls.h through the C-ABI
on the mock HIP runtime (tests/sanitize/mock_hip.cpp with its trace on): the covariance call, the
sampler, the mixture summaries on both scales, the trajectory targets, the component queries of a
resident factor, the self tests and the microbenchmarks, the scores of paths handed in and of paths
drawn on the device, the four long-horizon calls (prediction, paths, decomposition, hindcasts) on
factors with and without a main block, each at a small shape and each twice; then the sampler, the
targets, the path scores and the long-horizon calls with invalid arguments, one line
`call, fault: status` each; then the long-horizon calls on mock devices so small that the particles
go through in two or three chunks, where the driver also checks that every output element is
written and nothing around the outputs is.  Every
copy (kind, bytes, stream), kernel launch (mangled name, grid, block, LDS bytes, stream, integer
arguments) and event record of a call goes into one line, the number of records and their hash.
The output must equal tests/golden/oneshot_trace_v3.txt byte for byte: the host code around these
calls may be rearranged, what it asks of the runtime on a successful call may not change.  To see
WHAT moved, run the driver of two builds with --full and diff.  The golden file is regenerated only
by a change that means to move a copy or a launch.  No GPU is involved."""
import os
import subprocess

import pytest

from tests.test_host_sanitizers import HIPCC, ROOT, build

GOLDEN = os.path.join(ROOT, "tests", "golden", "oneshot_trace_v3.txt")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_oneshot_trace_equals_the_recorded_one(tmp_path):
    exe = build(str(tmp_path), [], "plain", "oneshot_trace")
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
