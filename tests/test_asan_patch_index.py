"""Patch format version 2 under AddressSanitizer + UBSan: `make asan-patch-index` builds tests/cpp/asan_patch_index.cpp (host_patch.cpp
and the host sources it needs in one translation unit with its own main) and drives the writer, the parser, add and strip over valid
patches of both versions, the hostile version-2 blobs of tests/patch_index_cases.py, every single-bit flip of a version-2 header, and
every patch at each of the 8 byte alignments of its index section, where the host's index reader -- the one
mpc_parse_container_by_index calls -- reads the section in place.  Each blob lies in a heap buffer of exactly its size.  Any sanitizer
report aborts the run; the driver also checks that whatever the parser accepts is byte for byte what the writer writes for what the
parser reports, and that a section read at any alignment yields the serial parse's symbols."""
import os
import subprocess

from conftest import ROOT


def test_patch_index_host_code_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "tests/cpp/asan_patch_index_bin"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_patch_index_bin")], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "asan_patch_index: 0 failed" in r.stdout and "asan_patch_index: 287194 cases" in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
