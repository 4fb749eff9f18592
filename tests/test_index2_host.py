"""Index version 2 on the host (no GPU): the aux section against its restatement in numpy (index2_cases), mpc_index_extend, the
windowed parse that cuts run-length packed and step-0 coefficient streams through it against slices of the serial parse, the
chunks it reads, the chunks it never reads, and damaged indexes.  Every equality is exact."""
import numpy as np
import pytest

import index2_cases as cases
import parse_cases
import region_cases
from region_cases import ACROSS_1024


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def f1_indexes(ia):
    """{interval: (version 1, version 2)} of F1"""
    return {i: (ia.container_index(cases.f1(), i), ia.container_index(cases.f1(), i, expanded=True)) for i in cases.F1_INTERVALS}


@pytest.fixture(scope="module")
def f2_indexes(ia):
    return ia.container_index(cases.f2(), cases.F2_INTERVAL), ia.container_index(cases.f2(), cases.F2_INTERVAL, expanded=True)


def _check_aux(ia, blob, interval, what):
    v1, v2 = ia.container_index(blob, interval), ia.container_index(blob, interval, expanded=True)
    assert ia.api.container_index2(blob, interval, 0) == v1, what
    assert ia.index_version(v1) == 1 and ia.index_version(v2) == 2, what
    assert v2[:4] == v1[:4] and v2[8:len(v1)] == v1[8:], what      # the version-1 part, but for the version word
    info1, info2 = ia.index_info(v1), ia.index_info(v2)
    assert info1["interval"] == info2["interval"] and len(info1["streams"]) == len(info2["streams"])
    for a, b in zip(info1["streams"], info2["streams"]):
        assert all(np.array_equal(a[key], b[key]) for key in a), what
    want = cases.expected_aux(blob, interval)
    entries = 0
    for j, exp in enumerate(want):
        got = ia.index_aux(v2, j)
        assert len(ia.index_aux(v1, j)["out"]) == 0, (what, j)
        if exp is None or info1["serial_only"]:
            assert len(got["out"]) == 0, (what, j)
            continue
        assert len(exp[0]) == len(info1["streams"][j]["checkpoints"]), (what, j)
        for key, arr in zip(("out", "prev", "state", "dc"), exp):
            assert got[key].dtype == arr.dtype and np.array_equal(got[key], arr), (what, j, key)
        entries += len(exp[0])
    assert len(v2) == len(v1) + 8 + 16 * entries, what
    assert int(np.frombuffer(v2[len(v1):len(v1) + 8], "<u8")[0]) == entries, what
    assert ia.index_extend(blob, v1) == v2, what
    assert ia.index_extend(blob, v2) == v2, what
    return v1, v2


def test_the_frames_cover_what_they_are_meant_to(ia):
    cases.check_coverage(ia)


@pytest.mark.parametrize("interval", cases.F1_INTERVALS)
def test_aux_of_f1(ia, interval):
    _check_aux(ia, cases.f1(), interval, ("F1", interval))


def test_aux_of_f2(ia):
    _check_aux(ia, cases.f2(), cases.F2_INTERVAL, "F2")


def test_aux_of_the_parse_cases(ia, oracle):
    for name, blob in list(parse_cases.synthetic().items()) + parse_cases.real(oracle):
        _check_aux(ia, blob, parse_cases.EDGE_INTERVAL, name)


def test_extend_from_a_damaged_index(ia, f1_indexes):
    blob = cases.f1()
    v1, v2 = f1_indexes[32]
    assert ia.index_extend(blob, v1) == v2
    info = ia.index_info(v1)
    head = 56 + 64 * len(info["streams"])
    for bit in (8 * head + 64 * 5 + 3, 8 * (len(v1) - 8) + 1, 8 * (56 + 64 * 3 + 16) + 2, 8 * (56 + 64 * 7 + 52), 8 * (56 + 64 * 9 + 56) + 4):
        assert ia.index_extend(blob, cases.flip(v1, bit)) == v2, bit    # a checkpoint, n_coded, mode and M: refused or corrected
    assert ia.index_extend(blob, v1[:len(v1) // 2]) == v2
    patched = bytearray(v1)
    patched[4] = 2                                                  # a version-1 blob that calls itself version 2 is no index
    assert ia.index_version(bytes(patched)) == 0
    assert ia.index_extend(blob, bytes(patched)) == v2
    with pytest.raises(ia.MpcError) as e:
        ia.index_extend(blob[:len(blob) // 2], v1)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM
    with pytest.raises(ia.MpcError) as e:
        ia.api.container_index2(blob, 32, 2)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT


def _window_cases(ia, f1_indexes, f2_indexes):
    """(name, container, height, interval, version 1, version 2, rectangles)"""
    out = [("F1", cases.f1(), region_cases.H, i, *f1_indexes[i], region_cases.RECTS) for i in cases.F1_INTERVALS]
    out.append(("F2", cases.f2(), cases.F2_SHAPE[1], cases.F2_INTERVAL, *f2_indexes, cases.F2_RECTS))
    return out


def test_window_parse_with_version_2(ia, f1_indexes, f2_indexes):
    for name, blob, height, interval, v1, v2, rects in _window_cases(ia, f1_indexes, f2_indexes):
        for rect in rects:
            want, want_ranges = region_cases.expected_window(blob, rect, height)
            for parse_all in (False, True):
                got, ranges, route = ia.parse_container_window_by_index(blob, v2, rect, parse_all)
                what = (name, interval, rect, parse_all)
                assert route == 0, what
                assert np.array_equal(ranges, want_ranges), what
                assert got.shape == want.shape and np.array_equal(got, want), what


def test_window_chunks(ia, f1_indexes, f2_indexes):
    whole_frame = {"F1": (0, 0, region_cases.W, region_cases.H), "F2": cases.F2_RECTS[0]}
    for name, blob, height, interval, v1, v2, rects in _window_cases(ia, f1_indexes, f2_indexes):
        k = ia.container_info(blob)[2]
        aux = cases.expected_aux(blob, interval)
        has = np.array([aux[i + 1] is not None for i in range(6 * k)])
        n_chunks = np.array([len(s["checkpoints"]) for s in ia.index_info(v1)["streams"][1:]], np.uint64)
        for rect in rects:
            what = (name, interval, rect)
            got2, route2 = ia.window_chunks_by_index(blob, v2, rect)
            got1, route1 = ia.window_chunks_by_index(blob, v1, rect)
            assert (route1, route2) == (0, 0), what
            assert np.array_equal(got2, cases.expected_chunks(blob, interval, rect, 2)), what
            assert np.array_equal(got1, cases.expected_chunks(blob, interval, rect, 1)), what
            assert np.array_equal(got1[has, 0], np.zeros(has.sum(), np.uint64)) and np.array_equal(got1[has, 1], n_chunks[has]), what
            assert np.array_equal(got1[~has], got2[~has]), what
            parsed1, parsed2 = int((got1[has, 1] - got1[has, 0]).sum()), int((got2[has, 1] - got2[has, 0]).sum())
            if rect != whole_frame[name]:
                assert parsed2 < parsed1, (what, parsed2, parsed1)
            else:
                assert parsed2 == parsed1, what
            for index in (v1, v2):
                every, route = ia.window_chunks_by_index(blob, index, rect, parse_all=True)
                assert route == 0 and np.array_equal(every[:, 0], np.zeros(6 * k, np.uint64)) and np.array_equal(every[:, 1], n_chunks), what
    none, route = ia.window_chunks_by_index(cases.f1(), b"not an index", ACROSS_1024)
    assert route == 1 and not none.any()


def _serial_answer(ia, damaged, rect, height):
    """what read_compressed gives for the damaged container: its window, or its refusal"""
    try:
        ia.read_compressed(damaged)
    except ia.MpcError:
        return None
    return region_cases.expected_window(damaged, rect, height)[0]


def test_chunks_outside_the_range_are_never_read(ia, f1_indexes):
    v1, v2 = f1_indexes[32]
    rect = ACROSS_1024
    want, _ = region_cases.expected_window(cases.f1(), rect, region_cases.H)
    for what, damaged in cases.never_read_containers(ia, v1):
        assert damaged != cases.f1()
        got, _, route = ia.parse_container_window_by_index(damaged, v2, rect)
        assert route == 0 and np.array_equal(got, want), what
        serial = _serial_answer(ia, damaged, rect, region_cases.H)
        for index, parse_all in ((v2, True), (v1, False), (v1, True)):
            if serial is None:
                with pytest.raises(ia.MpcError) as e:
                    ia.parse_container_window_by_index(damaged, index, rect, parse_all)
                assert e.value.status == ia.api.MPC_ERR_BITSTREAM, what
            else:
                got, _, route = ia.parse_container_window_by_index(damaged, index, rect, parse_all)
                assert np.array_equal(got, serial), (what, parse_all)
                assert route in (0, 1), what


def test_damaged_version_2_indexes(ia, oracle, f1_indexes):
    blob, rect = cases.f1(), ACROSS_1024
    v1, v2 = f1_indexes[32]
    want, want_ranges = region_cases.expected_window(blob, rect, region_cases.H)
    whole, _ = ia.parse_container_by_index(blob, v1)
    by_route = [0, 0]
    for what, bad in cases.damaged_v2(ia, oracle, v1, v2):
        got, ranges, route = ia.parse_container_window_by_index(blob, bad, rect, True)
        assert route in (0, 1) and np.array_equal(got, want) and np.array_equal(ranges, want_ranges), what
        got, ranges, route = ia.parse_container_window_by_index(blob, bad, rect)
        assert route in (0, 1), what
        by_route[route] += 1
        if route == 1:
            assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges), what
        chunks, _ = ia.window_chunks_by_index(blob, bad, rect)                                  # answers, whatever the index holds
        # a whole-frame parse uses nothing of the aux section beyond its structure
        got, route = ia.parse_container_by_index(blob, bad)
        assert route in (0, 1) and np.array_equal(got, whole), what
        if what.startswith("aux flip"):
            assert route == (0 if ia.index_version(bad) == 2 else 1), what
    assert by_route[0] >= 1 and by_route[1] >= 1, by_route


def test_exit_values_are_checked(ia, f1_indexes):
    blob, rect = cases.f1(), ACROSS_1024
    v1, v2 = f1_indexes[32]
    want, _ = region_cases.expected_window(blob, rect, region_cases.H)
    good = cases.expected_chunks(blob, 32, rect, 2)
    flips = cases.exit_flips(ia, blob, v2, v1, 32, rect)
    assert len(flips) >= 30 and {w.split()[4] for w, _ in flips} == {"out", "prev", "state", "dc"}
    caught = 0
    for what, bad in flips:
        i = int(what.split()[1])
        got, _, route = ia.parse_container_window_by_index(blob, bad, rect)
        chunks, chunks_route = ia.window_chunks_by_index(blob, bad, rect)
        if chunks_route == 0 and tuple(chunks[i]) != tuple(good[i]):
            assert route in (0, 1) and np.array_equal(got, want), what     # the flip moved c1: the damaged entry is no exit any more
            continue
        assert route == 1 and np.array_equal(got, want), what
        caught += 1
        # ... and a whole-frame parse does not care
        assert ia.parse_container_by_index(blob, bad)[1] == (0 if ia.index_version(bad) == 2 else 1), what
    assert caught >= 25, caught
