"""The windowed parse on the host (no GPU): mpc_parse_container_window_by_index, which defines what the region decoder's device
route computes, against slices of the serial parse expanded in numpy (region_cases), for good indexes, damaged ones and bad
arguments."""
import numpy as np
import pytest

import parse_cases
import region_cases
from region_cases import INTERVALS


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def _rects_for(w, h):
    """a few rectangles of any frame: whole, the corners' pixels, an odd one in the middle, a full-height band"""
    return [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 3 + 1, h // 3 + 2, max(w // 4, 1), max(h // 5, 1)),
            (w // 2, 0, min(9, w - w // 2), h)]


@pytest.fixture(scope="module")
def cases(ia, oracle):
    """[(name, container, height, rectangles)]"""
    out = [("region", region_cases.container(), region_cases.H, list(region_cases.RECTS))]
    for name, blob in list(parse_cases.synthetic().items()) + parse_cases.real(oracle):
        w, h, _, _ = ia.container_info(blob)
        out.append((name, blob, h, _rects_for(w, h)))
    return out


def test_the_frame_covers_what_it_is_meant_to(ia):
    region_cases.check_coverage(ia)
    # the numpy expansion is the library's own whole-frame expansion
    lengths, streams, _ = region_cases.expanded(region_cases.container())
    whole = ia.read_compressed(region_cases.container())
    assert np.array_equal(lengths, whole["lengths"])
    for mine, theirs in zip(streams, whole["codes"]):
        assert np.array_equal(mine, theirs)


def test_window_parse_equals_slices_of_the_serial_parse(ia, cases):
    for name, blob, height, rects in cases:
        for interval in INTERVALS:
            index = ia.container_index(blob, interval)
            for rect in rects:
                want, want_ranges = region_cases.expected_window(blob, rect, height)
                for parse_all in (False, True):
                    got, ranges, route = ia.parse_container_window_by_index(blob, index, rect, parse_all)
                    what = (name, interval, rect, parse_all)
                    assert route == 0, what
                    assert np.array_equal(ranges, want_ranges), what
                    assert got.shape == want.shape and np.array_equal(got, want), what


def test_the_whole_frame_window_is_the_whole_expansion(ia):
    blob = region_cases.container()
    lengths, streams, _ = region_cases.expanded(blob)
    got, ranges, route = ia.parse_container_window_by_index(blob, ia.container_index(blob, 32), region_cases.RECTS[0])
    assert route == 0 and np.array_equal(got, np.concatenate([lengths] + streams))
    assert (ranges[:, 0] == 0).all() and [int(r) for r in ranges[:, 1]] == [len(s) for s in streams[::2]]


def test_argument_errors(ia):
    blob = region_cases.container()
    index = ia.container_index(blob, 32)
    w, h = region_cases.W, region_cases.H
    for rect in ((0, 0, 0, 5), (0, 0, 5, 0), (3, 3, -1, 2), (-1, 0, 4, 4), (0, -1, 4, 4), (w, 0, 1, 1), (0, h, 1, 1), (w - 3, 0, 4, 1),
                 (0, h - 3, 1, 4), (0, 0, w + 1, h), (2 ** 31 - 1, 0, 2, 1)):
        with pytest.raises(ia.MpcError) as e:
            ia.parse_container_window_by_index(blob, index, rect)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, rect
    with pytest.raises(ia.MpcError) as e:
        ia.parse_container_window_by_index(blob[:len(blob) // 2], index, (0, 0, 1, 1))
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid input data")
    # an index that is none: route 1, the same result
    want, _ = region_cases.expected_window(blob, region_cases.ACROSS_1024, h)
    got, _, route = ia.parse_container_window_by_index(blob, b"no index at all", region_cases.ACROSS_1024)
    assert route == 1 and np.array_equal(got, want)


def test_damaged_indexes(ia, oracle, cases):
    """with "parse all" an index is a hint only; without, whatever passes the checks answers (status OK) and a refusal is exact"""
    others = dict(list(parse_cases.synthetic(1).items()) + parse_cases.real(oracle, seed=150))
    refused = [0, 0]
    for n, (name, blob, height, rects) in enumerate(cases):
        index = ia.container_index(blob, 32 if name == "region" else parse_cases.EDGE_INTERVAL)
        other = ia.container_index(others[name], parse_cases.EDGE_INTERVAL) if name in others else ia.container_index(blob, 64)
        rect = region_cases.ACROSS_1024 if name == "region" else rects[3]
        want, want_ranges = region_cases.expected_window(blob, rect, height)
        for what, bad in parse_cases.damaged_indexes(index, other, n):
            got, ranges, route = ia.parse_container_window_by_index(blob, bad, rect, True)
            assert route == ia.parse_container_by_index(blob, bad)[1], (name, what)
            assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges), (name, what)
            refused[1] += route
            got, ranges, route = ia.parse_container_window_by_index(blob, bad, rect, False)
            assert route in (0, 1), (name, what)
            if route == 1:
                assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges), (name, what)
            refused[0] += route
    assert refused[0] >= 1 and refused[1] >= refused[0]
