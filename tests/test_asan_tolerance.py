"""The change tolerance's host definition under AddressSanitizer + UBSan: `make asan-tolerance` builds tests/cpp/asan_tolerance.cpp
(host_delta.cpp in one translation unit, with its own main) and drives mpc::changed_tiles_tolerance on exact-size heap buffers -- every
width from 1 to 1041, the last row ending with the buffer, odd bases, padded rows whose padding differs, 0 against 255 everywhere, the
tolerances 0, 12 484 799, 12 484 800 and 2^32 - 1, with and without the sse array.  Any sanitizer report aborts the run."""
import os
import subprocess

from conftest import ROOT


def test_tolerance_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_tolerance_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_tolerance_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_tolerance: 0 failed" in r.stdout and "asan_tolerance: 1527 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
