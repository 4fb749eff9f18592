"""The delta encoder's host code under AddressSanitizer + UBSan: `make asan-delta` builds tests/cpp/asan_delta.cpp (host_delta.cpp in
one translation unit with its own main) and drives mpc::changed_tiles and mpc::pack_geometry over the shapes of delta_cases and the
extreme ones -- 1x1, a width that is no multiple of 8 with the minimum stride, n = 0 -- on exact-size buffers.  Any sanitizer report
aborts the run; the driver also checks the lists and the geometry."""
import os
import subprocess

from conftest import ROOT


def test_delta_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_delta_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_delta_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_delta: 0 failed" in r.stdout and "asan_delta: 836 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
