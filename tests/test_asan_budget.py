"""The rate control's host code under AddressSanitizer + UBSan: `make asan-budget` builds tests/cpp/asan_budget.cpp (host_budget.cpp with
the container's host sources in one translation unit, with its own main) and drives mpc::budget_lambda, mpc::budget_weights -- on the
seek indexes of the golden container and of random ones, whole, cut short, with bits flipped and sizes rewritten -- and
mpc::budget_allocate on exact-size buffers, counts above K among them.  Any sanitizer report aborts the run; the driver also checks
the weights against their definition and every allocation against a search over the depths."""
import os
import subprocess

from conftest import ROOT


def test_budget_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_budget_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_budget_bin"), os.path.join(ROOT, "tests", "golden", "r0c1de5e1t_3_5.mn")],
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_budget: 0 failed" in r.stdout and "asan_budget: 3170 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
