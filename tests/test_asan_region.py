"""The windowed parse's host code under AddressSanitizer + UBSan: `make asan-region` builds tests/cpp/asan_region.cpp (the host
sources in one translation unit, as `make asan-index` does) and drives mpc::read_window_by_index with damaged indexes, damaged
containers and rectangles of every kind; then the same binary takes the damaged inputs of tests/test_region_host.py and of
container_cases.corpus from files.  Any sanitizer report aborts the run; the driver also checks the trust rule's two halves."""
import os
import subprocess

import parse_cases
import region_cases
from container_cases import corpus
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_window_parse_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-region"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_region: 0 failed")
    import imageexperiments_amd as ia
    triples = []
    for n, blob, xs in corpus(oracle):
        index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
        w, h, _, _ = ia.container_info(blob)
        triples += [(x, index, (w // 3, h // 4, w - w // 3, h // 2 + 1)) for x in xs[::2]]
    assert len(triples) == 384
    others = dict(list(parse_cases.synthetic(1).items()) + parse_cases.real(oracle, seed=150))
    cases = [("region", region_cases.container())] + list(parse_cases.synthetic().items()) + parse_cases.real(oracle)
    for n, (name, blob) in enumerate(cases):
        index = ia.container_index(blob, 32 if name == "region" else parse_cases.EDGE_INTERVAL)
        other = ia.container_index(others[name], parse_cases.EDGE_INTERVAL) if name in others else ia.container_index(blob, 64)
        w, h, _, _ = ia.container_info(blob)
        rect = region_cases.ACROSS_1024 if name == "region" else (w // 3 + 1, h // 3 + 2, max(w // 4, 1), max(h // 5, 1))
        triples += [(blob, bad, rect) for _, bad in parse_cases.damaged_indexes(index, other, n)]
    for k, (x, index, rect) in enumerate(triples):
        (tmp_path / f"{k}.mn").write_bytes(x)
        (tmp_path / f"{k}.idx").write_bytes(index)
        (tmp_path / f"{k}.rect").write_text(" ".join(str(v) for v in rect))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_region_bin"), str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_region: {len(triples)} triples from files", "asan_region: 0 failed")
