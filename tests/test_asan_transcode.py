"""The transcode's host code under AddressSanitizer + UBSan: `make asan-transcode` builds tests/cpp/asan_transcode.cpp (the host
sources in one translation unit, as `make asan-view` does) and drives mpc::transcode_container on damaged containers and views of
every kind; then the same binary takes the damaged inputs of container_cases.corpus, and the transcode tests' rectangles and
argument errors on their frame, from files.  Any sanitizer report aborts the run; the driver also checks the verdicts, the
whole-frame identities and that transcodes compose."""
import os
import subprocess

import region_cases
import transcode_cases as tc
from container_cases import corpus
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_transcode_is_clean_under_asan_and_ubsan(oracle, tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-transcode"], cwd=ROOT, capture_output=True, text=True, timeout=900), "asan_transcode: 0 failed")
    import imageexperiments_amd as ia
    pairs = []
    for n, blob, xs in corpus(oracle):
        w, h, k, _ = ia.container_info(blob)
        tx, ty = -(-w // 8), -(-h // 8)
        inner = (8 * (tx // 3), 8 * (ty // 3), w - 8 * (tx // 3), 8 * max(ty // 3, 1))      # tile aligned, right edge the frame's
        pairs += [(x, (tc.WHOLE if j % 3 == 0 else inner) + (j % (k + 2),)) for j, x in enumerate(xs[n % 2::2])]
    assert len(pairs) == 384
    main = region_cases.container()
    good = len(tc.RECTS) * len(tc.STEPS)
    pairs += [(main, rect + (m,)) for rect in tc.RECTS for m in tc.STEPS]
    pairs += [(main, tuple(min(max(v, -2**31), 2**31 - 1) for v in rect) + (m,)) for rect, m, _ in tc.ARGUMENT_ERRORS]
    for k, (x, view) in enumerate(pairs):
        (tmp_path / f"{k}.mn").write_bytes(x)
        (tmp_path / f"{k}.view").write_text(" ".join(str(v) for v in view))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_transcode_bin"), str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=900, env=env)
    _clean(r, f"asan_transcode: {len(pairs)} pairs from files", "asan_transcode: 0 failed")
    made = int(r.stdout.split("pairs from files, ")[1].split(" transcoded")[0])
    assert made >= good + 8, made
