"""The emphasis maps' host code under AddressSanitizer + UBSan: `make asan-emphasis` builds tests/cpp/asan_emphasis.cpp (host_budget.cpp
and host_rate.cpp with the container's host sources in one translation unit, with its own main) and drives mpc::budget_allocate_emphasis,
mpc::budget_sweep_emphasis, mpc::budget_allocate_floor_emphasis and mpc::emphasis_from_mask on exact-size heap buffers -- maps of every
byte value, profiles inside their bounds, at them and far outside, counts above K, list entries outside the frame, masks of widths 1 to
4928 whose last row ends with the buffer, at odd bases and with padded rows.  Any sanitizer report aborts the run."""
import os
import subprocess

from conftest import ROOT


def test_emphasis_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_emphasis_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_emphasis_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_emphasis: 0 failed" in r.stdout and "asan_emphasis: 228 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
