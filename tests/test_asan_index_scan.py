"""The seek index from a bit scan under AddressSanitizer + UBSan: `make asan-index-scan` builds tests/cpp/asan_index_scan.cpp (the
host sources in one translation unit, as `make asan-host` does) and drives mpc_container_index_scan's host code -- step table,
segment maps, chain, walk, the proposal and its acceptance -- with damaged and truncated containers, the reference's own .mn among
them, at sizes that make codes span segments and streams span windows; then the same binary takes container_cases.corpus from
files.  Any sanitizer report aborts the run; the driver also checks that every verdict and blob is the serial builder's and that the
scan does not give up where the serially built index is one the chunked parse uses."""
import os
import subprocess

from container_cases import corpus
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_index_scan_code_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-index-scan"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_index_scan: 0 failed")
    xs = [x for _, _, damaged in corpus(oracle) for x in damaged]
    assert len(xs) == 768
    for k, x in enumerate(xs):
        (tmp_path / f"{k}.mn").write_bytes(x)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_index_scan_bin"), "", str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_index_scan: {len(xs)} containers from files", "asan_index_scan: 0 failed")
