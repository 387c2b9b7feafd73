"""The host code of ngp_factor_sample_long_indep and the body it shares with
ngp_factor_sample_long (argument checks, the limits at the bound and one over, chunking of the items
on a small device, the runs of items that carry weight, two threads on one factor, one in each
form) under ThreadSanitizer and AddressSanitizer + UBSan, against the mock HIP runtime: the build of
tests/test_host_sanitizers.py with the driver tests/sanitize/sample_long_indep_stress.cpp."""
import os
import subprocess

import pytest

from tests.test_host_sanitizers import HIPCC, build


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
@pytest.mark.parametrize("tag,flags,env", [
    ("tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=0 report_signal_unsafe=0"}),
    ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
     {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}),
])
def test_sample_long_indep_under_sanitizers(tmp_path, tag, flags, env):
    exe = build(str(tmp_path), flags, tag, "sample_long_indep_stress")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env={**os.environ, **env})
    report = out.stdout[-3000:] + out.stderr[-6000:]
    assert "ThreadSanitizer" not in out.stderr, report
    assert "AddressSanitizer" not in out.stderr and "LeakSanitizer" not in out.stderr, report
    assert "runtime error" not in out.stderr, report
    assert out.returncode == 0, report
    assert "0 failures" in out.stdout, report
