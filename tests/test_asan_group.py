"""The group encodes' host code under AddressSanitizer + UBSan: `make asan-group` builds tests/cpp/asan_group.cpp (host_budget.cpp and
host_codec.cpp with the container's host sources in one translation unit, with its own main) and drives mpc::budget_allocate_group and
mpc::budget_sweep_group on exact-size buffers against the single-frame functions frame by frame -- 1 to 64 frames, profiles inside their
bounds, at them and far outside, counts above K, any byte in the map -- and mpc::sse_for_psnr over mpc::psnr_from_sse_pixels against its
neighbours.  Any sanitizer report aborts the run."""
import os
import subprocess

from conftest import ROOT


def test_group_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_group_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_group_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_group: 0 failed" in r.stdout and "asan_group: 1727 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
