"""The views' host code under AddressSanitizer + UBSan: `make asan-view` builds tests/cpp/asan_view.cpp (the host sources in one
translation unit, as `make asan-region` does) and drives mpc::truncate_container and mpc::read_window_by_index with `steps` on
damaged indexes, damaged containers and views of every kind; then the same binary takes the damaged inputs of
container_cases.corpus and the damaged indexes of the view tests from files.  Any sanitizer report aborts the run; the driver also
checks that a view's parse is the windowed parse of the truncated container and the trust rule's two halves."""
import os
import subprocess

import parse_cases
import region_cases
import view_cases
from container_cases import corpus
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_views_are_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-view"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_view: 0 failed")
    import imageexperiments_amd as ia
    triples = []
    for n, blob, xs in corpus(oracle):
        w, h, k, _ = ia.container_info(blob)
        for version in (1, 2):
            index = ia.container_index(blob, parse_cases.EDGE_INTERVAL, expanded=version == 2)
            triples += [(x, index, (w // 3, h // 4, w - w // 3, h // 2 + 1, 1 + (j + version) % (k + 1))) for j, x in enumerate(xs[version - 1::4])]
    assert len(triples) == 384
    main = view_cases.main()
    other = bytes(oracle.OracleContext(region_cases.K, 8, region_cases.QUALITY).encode_image(oracle.synth_frame(region_cases.W, region_cases.H, 778)))
    for version in (1, 2):
        index = ia.container_index(main, 32, expanded=version == 2)
        twin = ia.container_index(other, 32, expanded=version == 2)
        for j, (_, bad) in enumerate(parse_cases.damaged_indexes(index, twin, version)):
            rect = (view_cases.RECTS + (view_cases.UNALIGNED,))[j % 7]
            triples.append((main, bad, rect + ((0, 1, 2, 3, 8, 9)[j % 6],)))
    damaged = view_cases.flip_in_stream(main, ia.container_index(main, 32), 2 * region_cases.K)
    triples += [(damaged, ia.container_index(main, 32, expanded=version == 2), (0, 0, region_cases.W, region_cases.H, m))
                for version in (1, 2) for m in (1, 2, 7, 8)]
    for k, (x, index, view) in enumerate(triples):
        (tmp_path / f"{k}.mn").write_bytes(x)
        (tmp_path / f"{k}.idx").write_bytes(index)
        (tmp_path / f"{k}.view").write_text(" ".join(str(v) for v in view))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_view_bin"), str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_view: {len(triples)} triples from files", "asan_view: 0 failed")
