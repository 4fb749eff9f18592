"""The target-quality encode's host code under AddressSanitizer + UBSan: `make asan-quality` builds tests/cpp/asan_quality.cpp
(host_budget.cpp and host_codec.cpp with the container's host sources in one translation unit, with its own main) and drives
mpc::budget_sweep on exact-size buffers against mpc::budget_allocate at all 256 multipliers, mpc::quality_pick against its definition
and mpc::sse_for_psnr over mpc::psnr_from_sse against its neighbours -- on profiles inside their bounds, at them and far outside,
counts above K, totals no sweep makes and PSNR targets of every kind.  Any sanitizer report aborts the run."""
import os
import subprocess

from conftest import ROOT


def test_quality_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_quality_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_quality_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_quality: 0 failed" in r.stdout and "asan_quality: 2173 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
