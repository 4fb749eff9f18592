"""Index version 2's host code under AddressSanitizer + UBSan: `make asan-index2` builds tests/cpp/asan_index2.cpp (the host
sources in one translation unit, a stand-alone program) and drives the aux section's builder and reader, mpc::extend_container_index
and mpc::read_window_by_index with damaged indexes and damaged containers; then the same binary takes the damaged version-2
indexes and the bit-flipped containers of tests/test_index2_host.py from files.  Any sanitizer report aborts the run; the driver
also checks the trust rule's two halves."""
import os
import subprocess

import index2_cases as cases
import region_cases
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_index_version_2_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-index2"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_index2: 0 failed")
    import imageexperiments_amd as ia
    blob, rect = cases.f1(), region_cases.ACROSS_1024
    v1, v2 = ia.container_index(blob, 32), ia.container_index(blob, 32, expanded=True)
    triples = [(blob, bad, rect) for _, bad in cases.damaged_v2(ia, oracle, v1, v2) + cases.exit_flips(ia, blob, v2, v1, 32, rect)]
    triples += [(x, index, rect) for _, x in cases.never_read_containers(ia, v1) for index in (v1, v2)]
    f2v1, f2v2 = ia.container_index(cases.f2(), cases.F2_INTERVAL), ia.container_index(cases.f2(), cases.F2_INTERVAL, expanded=True)
    triples += [(cases.f2(), bad, cases.F2_INNER) for _, bad in cases.damaged_aux(ia, f2v2, f2v1, 3, count=16)]
    assert len(triples) > 150
    for k, (x, index, r) in enumerate(triples):
        (tmp_path / f"{k}.mn").write_bytes(x)
        (tmp_path / f"{k}.idx").write_bytes(index)
        (tmp_path / f"{k}.rect").write_text(" ".join(str(v) for v in r))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_index2_bin"), str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_index2: {len(triples)} triples from files", "asan_index2: 0 failed")
