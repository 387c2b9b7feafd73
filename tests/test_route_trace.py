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


GRAMMAR_GOLDEN = os.path.join(ROOT, "tests", "golden", "route_trace_grammar_v1.txt")
GRAMMAR_ZOO = os.path.join(ROOT, "tests", "golden", "grammar_zoo_v1.txt")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("route_trace")), [], "plain", "route_trace")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_grammar_zoo_launches_every_contraction_instantiation(driver):
    """`route_trace --grammar`: the batches of tests/test_grammar_gpu.py whose contraction kernel the
    kernel-class profile cannot show.  Byte for byte against the recorded trace, and in clear: the six
    G-sized prefixes (largest tree 1, 3, 7, 15, 31, 63 operators) launch six different contraction
    kernels — the lists kernel for 1, 2, 4, 8 leaves, its two passes for 16, the lattice kernel
    beyond — the batch-invariant run launches all of them, and the Toeplitz prefixes launch the DIAG
    instantiations (last template argument true) for 1, 2, 4, 8 and 16 leaves."""
    out = subprocess.run([driver, "--grammar", GRAMMAR_ZOO], capture_output=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:].decode() + out.stderr[-2000:].decode()
    calls, head = {}, None
    for ln in out.stdout.decode().splitlines():
        if ln.startswith("== "):
            head = ln
        elif " records #" in ln and head:
            calls.setdefault(head.split(" n=")[0][3:], []).append(
                {w for w in ln.replace(",", " ").split() if "grad_contract" in w})
    sized = calls["G-sized"]
    assert len(sized) == 6 and all(len(k) >= 1 for k in sized), sized
    assert len({frozenset(k) for k in sized}) == 6, sized

    def lists(nl, nacc, pas, diag):
        return f"grad_contract_listsILi{nl}ELi{nacc}ELi{pas}ELb{diag}E["
    want = [{lists(1, 1, 0, 0)}, {lists(2, 2, 0, 0)}, {lists(4, 4, 0, 0)}, {lists(8, 8, 0, 0)},
            {lists(16, 8, 0, 0), lists(16, 8, 1, 0)}, {"grad_contract_latticeILb0E["}]
    for got, w in zip(sized, want):
        assert len(got) == len(w) and all(any(x in g for g in got) for x in w), (got, w)
    own, = calls["G-own"]
    assert all(any(x in g for g in own) for w in want for x in w), own
    toep = calls["G-toep"]
    assert len(toep) == 5
    for got, nl in zip(toep, (1, 2, 4, 8, 16)):
        assert got and all(f"grad_contract_listsILi{nl}ELi" in g and "Lb1E[" in g for g in got), (nl, got)
    assert all("Lb1E[" not in g for g in calls["G-toep with the 17-leaf tree"][0])
    with open(GRAMMAR_GOLDEN, "rb") as f:
        assert out.stdout == f.read()


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_launch_trace_equals_the_recorded_one(driver):
    exe = driver
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
