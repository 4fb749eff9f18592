"""The compose's host code under AddressSanitizer + UBSan: `make asan-compose` builds tests/cpp/asan_compose.cpp (the host sources in
one translation unit, as `make asan-transcode` does) and drives mpc::compose_container on damaged containers and part lists of every
kind; then the same binary takes the damaged inputs of container_cases.corpus, as the base and as an overlay, and the compose tests'
part lists and argument errors, from files.  Any sanitizer report aborts the run; the driver also checks the verdicts and the
quadrant identity."""
import os
import subprocess

import compose_cases as cc
from container_cases import corpus
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _clamp(v):
    return min(max(int(v), -2**31), 2**31 - 1)


def test_compose_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-compose"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_compose: 0 failed")
    import imageexperiments_amd as ia
    cases = []                                                      # (blobs, parts, width, height, expected verdict or -1)
    for n, blob, xs in corpus(oracle):
        w, h, _, _ = ia.container_info(blob)
        tx, ty = -(-w // 8), -(-h // 8)
        corner = (8 * (tx - 1), 8 * (ty - 1), w - 8 * (tx - 1), h - 8 * (ty - 1))
        for j, x in enumerate(xs[n % 2::4]):
            overlay = (1, corner, corner[0], corner[1])
            # damaged as the base, as an overlay, and named only by a part that owns nothing
            lists = (((x, blob), ((0, None, 0, 0), overlay)), ((blob, x), ((0, None, 0, 0), overlay)), ((blob, x), ((1, None, 0, 0), (0, None, 0, 0))))
            blobs, parts = lists[j % 3]
            cases.append((blobs, parts, w, h, -1))
    assert len(cases) == 192
    good = 0
    for name in cc.NAMES:
        blobs, parts, width, height = cc.lists()[name]
        cases.append((blobs, parts, width, height, 0))
        good += 1
    for names, parts, width, height, _, _ in cc.ARGUMENT_ERRORS:
        cases.append(([cc.named(n) for n in names], parts, width, height, 2))
    cases.append(((cc.container(), cc.length_above_K()), ((0, None, 0, 0), (1, (0, 0, 8, 8), 0, 0)), cc.W, cc.H, 1))
    for k, (blobs, parts, width, height, expect) in enumerate(cases):
        for s, x in enumerate(blobs):
            (tmp_path / f"{k}.{s}.mn").write_bytes(x)
        lines = [f"{len(blobs)} {len(parts)} {width} {height} {expect}"]
        lines += [" ".join(str(_clamp(v)) for v in (source,) + tuple(rect or (0, 0, 0, 0)) + (x, y)) for source, rect, x, y in parts]
        (tmp_path / f"{k}.case").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_compose_bin"), str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_compose: {len(cases)} cases from files", "asan_compose: 0 failed")
    made = int(r.stdout.split("cases from files, ")[1].split(" composed")[0])
    assert made >= good + 8, made
