"""The copies, memsets, launches and synchronisations of the staged runs against a recorded trace.

tests/sanitize/staged_trace.cpp walks the sequences of tests/sanitize/staged_calls.h through the
C-ABI on the mock HIP runtime (tests/sanitize/mock_hip.cpp with its trace on): value jobs staged,
run, run again and fetched (packed and unpacked results, mixed precision with refinement, no main
block), a resident factor made and queried, gradient jobs run with new parameters on one leaf and on
two leaves side by side, trajectories with and without a trace.  Per step the number of records,
their hash, the number of streams that saw a launch and the number of synchronisations must equal
tests/golden/staged_trace_v1.txt byte for byte: the host code around the staged runs may be
rearranged, what it asks of the runtime on a successful run — host round trips included — may not
change.  To see WHAT moved, run the driver of two builds with --full and diff.  The golden file is
regenerated only by a change that means to move a copy, a launch or a synchronisation.  No GPU is
involved."""
import os
import subprocess

import pytest

from tests.test_host_sanitizers import HIPCC, ROOT, build

GOLDEN = os.path.join(ROOT, "tests", "golden", "staged_trace_v1.txt")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_staged_trace_equals_the_recorded_one(tmp_path):
    exe = build(str(tmp_path), [], "plain", "staged_trace")
    out = subprocess.run([exe], capture_output=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:].decode() + out.stderr[-2000:].decode()
    with open(GOLDEN, "rb") as f:
        want = f.read()
    got = out.stdout
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        head = next((ln for ln in reversed(g[:k + 1]) if ln.startswith(b"--")), b"")
        pytest.fail(f"trace differs from line {k + 1} ({len(g)} lines against {len(w)}), in {head.decode()} "
                    f"(run the driver with --full for the records):\n"
                    f"  got  {g[k].decode() if k < len(g) else '<end>'}\n"
                    f"  want {w[k].decode() if k < len(w) else '<end>'}")
