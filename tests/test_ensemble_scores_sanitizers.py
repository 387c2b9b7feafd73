"""The path scores' host code (validation, limits, staging, the fold of the partial sums, frees on
every error return, the context's lock) under AddressSanitizer + UBSan, against the mock HIP
runtime: the build of tests/test_host_sanitizers.py with the driver
tests/sanitize/ensemble_scores_stress.cpp, a stand-alone program with its own main."""
import os
import subprocess

import pytest

from tests.test_host_sanitizers import HIPCC, build


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_ensemble_scores_under_asan_and_ubsan(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = build(str(tmp_path), flags, "asan", "ensemble_scores_stress")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1",
                              "UBSAN_OPTIONS": "print_stacktrace=1"})
    report = out.stdout[-3000:] + out.stderr[-6000:]
    assert "AddressSanitizer" not in out.stderr and "LeakSanitizer" not in out.stderr, report
    assert "runtime error" not in out.stderr, report
    assert out.returncode == 0, report
    assert "0 failures" in out.stdout, report
