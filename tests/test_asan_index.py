"""The seek index's host code under AddressSanitizer + UBSan: `make asan-index` builds tests/cpp/asan_index.cpp (the host sources
in one translation unit, as `make asan-host` does) and drives the index builder, the validator (on one thread and on the worker
pool) and the host's chunk decoder with damaged containers and damaged indexes, the reference's own .mn among them; then the
same binary takes the inputs of tests/test_container_index.py from files: container_cases.corpus with the undamaged container's
index, and parse_cases.damaged_indexes of A - E.  Any sanitizer report aborts the run; the driver also checks that every result
is the serial parse's."""
import os
import subprocess

import parse_cases
from container_cases import corpus
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_index_code_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-index"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_index: 0 failed")
    import imageexperiments_amd as ia
    pairs = []
    for n, blob, xs in corpus(oracle):
        index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
        pairs += [(x, index) for x in xs]
    assert len(pairs) == 768
    others = dict(list(parse_cases.synthetic(1).items()) + parse_cases.real(oracle, seed=150))
    for n, (name, blob) in enumerate(list(parse_cases.synthetic().items()) + parse_cases.real(oracle)):
        index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
        other = ia.container_index(others[name], parse_cases.EDGE_INTERVAL)
        pairs += [(blob, bad) for _, bad in parse_cases.damaged_indexes(index, other, n)]
    for k, (x, index) in enumerate(pairs):
        (tmp_path / f"{k}.mn").write_bytes(x)
        (tmp_path / f"{k}.idx").write_bytes(index)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_index_bin"), "", str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_index: {len(pairs)} pairs from files", "asan_index: 0 failed")
