"""The delta stream's patch format under AddressSanitizer + UBSan: `make asan-patch` builds tests/cpp/asan_patch.cpp (host_patch.cpp and
the host sources it needs in one translation unit with its own main) and drives the one writer and the one parser over valid patches
of the three forms, the hostile corpus of tests/patch_cases.py and every single-bit flip of valid patches' headers and lists, each on
a heap buffer of exactly the blob's size.  Any sanitizer report aborts the run; the driver also checks that whatever the parser accepts
is byte for byte what the writer writes for what the parser reports."""
import os
import subprocess

from conftest import ROOT


def test_patch_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_patch_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_patch_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_patch: 0 failed" in r.stdout and "asan_patch: 4463 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
