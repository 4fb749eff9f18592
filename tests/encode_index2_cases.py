"""Inputs for the tests of index version 2 as the encoder emits it, shared by the host tests and the device tests (nothing here
needs a GPU).  A case is what encode_index_cases describes: dict(W, H, K, quant, counts, streams), the streams as coded.

main2()   encode_index_cases.main() with its three step-0 coefficient streams (1, 2K + 1, 4K + 1) replaced by streams that come out
          run-length packed: long runs around the entropy stage's 4096-symbol blocks and the run-length cut at 0x8001, and two
          kinds of short runs
main      encode_index_cases.main() itself: the step-0 streams unpacked, eleven other streams packed
f1, f2    the streams of index2_cases' two oracle frames handed back as coded (all three step-0 streams packed; two of three not)
C, D      encode_index_cases.synthetic: nothing packed

check_coverage asserts what each case is there for from container_index(..., expanded=True) and index2_cases.aux_of, so a changed
input fails there instead of testing nothing."""
import functools

import numpy as np

import encode_index_cases as v1_cases
import index2_cases
from encode_index_cases import K, LENGTHS, _contents, assemble

INTERVALS = v1_cases.INTERVALS                                      # 0, 32, 33, 100, 128, 4096, 4097, 65536
LONG_RUNS = (0x8002, 4097, 0x8001, 4096, 0x8003, 4095, 0x8000)
STEP0 = (1, 2 * K + 1, 4 * K + 1)
MAIN2_CODED = (1440, 9016, 6957)                                    # coded symbols of main2's step-0 streams, all packed
NAMES = ("main2", "main", "f1", "f2", "C", "D")
_FIELDS = ("out", "prev", "state", "dc")


@functools.lru_cache(maxsize=None)
def main2():
    rng = np.random.default_rng(20250403)
    case = dict(v1_cases.main())
    streams = list(case["streams"])
    n = LENGTHS[0][0]
    parts = []
    for length in LONG_RUNS:
        parts.append(np.full(length, rng.integers(1, 65536)))
        parts.append(np.repeat(rng.integers(0, 65536, 150), rng.integers(1, 4, 150)))
    streams[1] = np.concatenate(parts)[:n].astype(np.uint16)
    assert len(streams[1]) == n
    streams[2 * K + 1] = np.asarray(_contents(2, LENGTHS[1][0], rng), np.int64).astype(np.uint16)
    streams[4 * K + 1] = np.asarray(_contents(7, LENGTHS[2][0], rng), np.int64).astype(np.uint16)
    case["streams"] = streams
    return case


@functools.lru_cache(maxsize=None)
def case(name):
    import imageexperiments_amd as ia
    if name == "main2":
        return main2()
    if name == "main":
        return v1_cases.main()
    if name in ("f1", "f2"):
        return v1_cases.from_container(ia, index2_cases.f1() if name == "f1" else index2_cases.f2())
    return v1_cases.synthetic(name)


@functools.lru_cache(maxsize=None)
def container(name):
    """the case's container by the direct host route"""
    import imageexperiments_amd as ia
    return assemble(ia, case(name))


def _packed(ia, blob):
    return [bool(p) for p in ia.read_compressed(blob, coded=True)["packed"]]


def _states(blob, interval, stream):
    """the states of a packed stream's entries, from the numpy restatement"""
    return {int(s) for s in index2_cases.expected_aux(blob, interval)[stream + 1][2]}


def check_coverage(ia):
    """what the cases are there for"""
    # main2: the long runs
    blob = container("main2")
    assert assemble(ia, main2(), by_plan=True) == blob
    coded = ia.read_compressed(blob, coded=True)
    assert [bool(coded["packed"][i]) for i in STEP0] == [True, True, True]
    assert tuple(len(coded["codes"][i]) for i in STEP0) == MAIN2_CODED
    for interval in (32, 33, 100, 128):
        assert _states(blob, interval, 1) == {0, 1, 2}, interval
    out, prev, state, dc = index2_cases.expected_aux(blob, 32)[2]
    parsed = ia.index_aux(ia.container_index(blob, 32, expanded=True), 2)      # the host's own pass agrees with the restatement
    assert all(np.array_equal(parsed[k], v) for k, v in zip(_FIELDS, (out, prev, state, dc)))
    steps = np.diff(out.astype(np.int64))
    assert int((steps > 0x8001).sum()) == 2 and int((steps > 4096).sum()) == 4      # whole blocks and a chunk cut inside an interval
    assert len(set(int(x) for x in dc)) == len(dc)                  # a wrong sum cannot hide behind an equal neighbour
    total = int(index2_cases.zigzag(main2()["streams"][1]).sum())
    assert abs(total) > 1 << 16                                     # the 16 bits kept of the sums wrap
    # main: the step-0 streams unpacked, the others of every kind
    blob = container("main")
    packed = _packed(ia, blob)
    assert [packed[i] for i in STEP0] == [False, False, False] and sum(packed) == 11
    for interval in (32, 33, 128, 4097):
        seen = set()
        for i in range(6 * K):
            if packed[i]:
                seen |= _states(blob, interval, i)
        assert seen == {0, 1, 2}, interval
    assert 0 in [len(s) for s in v1_cases.main()["streams"]]
    # f1, f2: the oracle's frames
    k1 = ia.container_info(index2_cases.f1())[2]
    packed = _packed(ia, container("f1"))
    assert sum(packed) == 28 and all(packed[i] for i in (1, 2 * k1 + 1, 4 * k1 + 1))
    k2 = ia.container_info(index2_cases.f2())[2]
    packed = _packed(ia, container("f2"))
    assert [packed[i] for i in (1, 2 * k2 + 1, 4 * k2 + 1)] == [False, False, True]
    for name in ("C", "D"):
        assert not any(_packed(ia, container(name))), name


def first_difference(ia, got, want):
    """where two indexes of one container differ, for an assertion's message: the version-1 part by
    encode_index_cases.first_difference, then the first differing stream, entry and field of the aux section"""
    if got == want:
        return "equal"
    if got is None or want is None:
        return v1_cases.first_difference(ia, got, want)
    try:
        versions = ia.index_version(got), ia.index_version(want)
        if versions[0] != versions[1]:
            return f"version {versions[0]} against {versions[1]}"
        head = v1_cases.first_difference(ia, got, want)
        if not head.startswith("sizes"):
            return head
        for j in range(1, len(ia.index_info(want)["streams"])):
            a, b = ia.index_aux(got, j), ia.index_aux(want, j)
            if len(a["out"]) != len(b["out"]):
                return f"stream {j}: {len(a['out'])} aux entries against {len(b['out'])}"
            for name in _FIELDS:
                bad = np.nonzero(a[name] != b[name])[0]
                if bad.size:
                    return f"stream {j} aux entry {bad[0]} field {name}: {a[name][bad[0]]} against {b[name][bad[0]]}"
        return head
    except ia.MpcError as e:
        return f"not an index: {e}"
