"""Index version 2 as the encoder emits it, on the host under AddressSanitizer + UBSan: `make asan-encode-index2` builds
tests/cpp/asan_encode_index2.cpp (the host sources in one translation unit, as `make asan-index` does) and runs the by-plan route
that computes the aux entries and index_from_plan, which checks them, on random streams and on aux arrays that contradict the
plans; then the same binary takes the stream cases of tests/test_encode_index2_host.py from files (main2, main, the two oracle
frames, parse_cases' D, the inconsistent streams of stream_cases).  Any sanitizer report aborts the run; the driver also checks
every container against the direct route and every index against the parsed one.  Nothing is loaded into python under a
sanitizer."""
import os
import struct
import subprocess

import numpy as np

import encode_index2_cases as cases
import stream_cases
from conftest import ROOT


def _clean(r, *lines):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for line in lines:
        assert line in r.stdout, r.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _write(path, case):
    k = case["K"]
    streams = [np.ascontiguousarray(x, np.uint16).ravel() for x in case["streams"]]
    off = np.zeros(6 * k + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in streams])
    counts = np.ascontiguousarray(case["counts"], np.uint16).ravel()
    with open(path, "wb") as f:
        f.write(struct.pack("<3I", case["W"], case["H"], k))
        f.write(np.ascontiguousarray(case["quant"], np.float64).reshape(3 * k).tobytes())
        f.write(struct.pack("<Q", counts.size))
        f.write(counts.tobytes())
        f.write(off.tobytes())
        f.write(struct.pack("<Q", int(off[-1])))
        f.write(np.concatenate(streams).tobytes() if int(off[-1]) else b"")


def test_encode_index2_code_is_clean_under_asan_and_ubsan(tmp_path):
    _clean(subprocess.run(["make", "-s", "asan-encode-index2"], cwd=ROOT, capture_output=True, text=True, timeout=900),
           "asan_encode_index2: 0 failed")
    odd = stream_cases.make()
    inputs = [cases.case(name) for name in ("main2", "main", "f1", "f2", "D")] + [
              dict(W=odd["W"], H=odd["H"], K=odd["K"], quant=stream_cases.quant(odd["K"]), counts=odd["counts"], streams=odd["as_coded"])]
    for k, case in enumerate(inputs):
        _write(tmp_path / f"{k}.case", case)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", MPC_HOST_THREADS="4")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_encode_index2_bin"), str(tmp_path)], cwd=ROOT, capture_output=True,
                       text=True, timeout=900, env=env)
    _clean(r, f"asan_encode_index2: {len(inputs)} cases from files", "asan_encode_index2: 0 failed")
