"""Views on the host (no GPU): mpc_truncate_container against the oracle's reader and writer, and
mpc_parse_container_view_by_index -- which defines what the view decoder's device route parses -- against the windowed parse of the
truncated container (region_cases.expected_window), for good indexes, damaged ones and bad arguments.  Every equality is exact."""
import numpy as np
import pytest

import parse_cases
import region_cases
import view_cases
from container_cases import corpus as _corpus


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def inputs(oracle):
    """[(name, container, K)]"""
    return [("main", view_cases.main(), region_cases.K), ("small", view_cases.small(), view_cases.SMALL_K)]


def test_truncation_is_the_oracles(ia, oracle, inputs):
    for name, blob, k in inputs:
        assert ia.container_info(blob)[2] == k
        sizes = []
        for m in range(1, k + 1):
            got = ia.truncate_container(blob, m)
            assert got == view_cases.truncated(blob, m), (name, m)
            assert ia.container_info(got) == ia.container_info(blob)
            sizes.append(len(got))
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], name
        for m in (k, k + 5):
            assert ia.truncate_container(blob, m) == blob, (name, m)
        for m in (0, -1):
            with pytest.raises(ia.MpcError) as e:
                ia.truncate_container(blob, m)
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT, (name, m)


def test_truncated_streams_are_the_cut_streams(ia, inputs):
    for name, blob, k in inputs:
        whole = ia.read_compressed(blob)
        for m in (1, 2, k - 1):
            cut = ia.read_compressed(ia.truncate_container(blob, m))
            assert np.array_equal(cut["lengths"], np.minimum(whole["lengths"], m)) and np.array_equal(cut["quant"], whole["quant"])
            for i in range(6 * k):
                want = whole["codes"][i] if (i % (2 * k)) // 2 < m else np.zeros(0, np.uint16)
                assert np.array_equal(cut["codes"][i], want), (name, m, i)


def test_truncation_refuses_what_read_compressed_refuses(ia, oracle):
    for n, blob, xs in _corpus(oracle):
        refused = 0
        for k, x in enumerate(xs):
            try:
                ia.read_compressed(x)
            except ia.MpcError:
                with pytest.raises(ia.MpcError) as e:
                    ia.truncate_container(x, 1)
                assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid input data"), (n, k)
                refused += 1
            else:
                ia.truncate_container(x, 1)
        assert refused > 10, n


def _indexes(ia, blob):
    """{(version, interval): index}"""
    return {(version, interval): ia.container_index(blob, interval, expanded=version == 2) for version in (1, 2) for interval in (32, 0)}


def test_view_parse_is_the_window_parse_of_the_truncation(ia, inputs):
    for name, blob, k in inputs:
        steps = view_cases.PARSE_STEPS if name == "main" else (1, 5, 32, 0)
        rects = view_cases.PARSE_RECTS if name == "main" else (view_cases.WHOLE, (8, 8, 17, 9))
        for (version, interval), index in _indexes(ia, blob).items():
            for m in steps:
                for rect in rects:
                    want, want_ranges = view_cases.expected_parse(blob, rect, m, k)
                    for parse_all in (False, True):
                        got, ranges, route = ia.parse_container_view_by_index(blob, index, (rect, m, 0), parse_all)
                        what = (name, version, interval, m, rect, parse_all)
                        assert route == 0, what
                        assert np.array_equal(ranges, want_ranges), what
                        assert got.shape == want.shape and np.array_equal(got, want), what
                        if 0 < m < k:                               # streams of steps at or above m: empty
                            assert not ranges[[ch * k + i for ch in range(3) for i in range(m, k)]].any(), what


def test_steps_zero_is_the_window_parse(ia):
    blob = view_cases.main()
    index = ia.container_index(blob, 32)
    for rect in region_cases.RECTS:
        want = ia.parse_container_window_by_index(blob, index, rect)
        got = ia.parse_container_view_by_index(blob, index, (rect, 0, 0))
        assert got[2] == want[2] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), rect


def test_damaged_indexes_take_route_one(ia, oracle):
    blob = view_cases.main()
    index = ia.container_index(blob, 32)
    other = ia.container_index(bytes(oracle.OracleContext(region_cases.K, 8, region_cases.QUALITY).encode_image(
        oracle.synth_frame(region_cases.W, region_cases.H, 778))), 32)
    rect, m = region_cases.ACROSS_1024, 2
    want, want_ranges = view_cases.expected_parse(blob, rect, m, region_cases.K)
    refused = 0
    for what, bad in parse_cases.damaged_indexes(index, other, 0) + [("none", b"no index at all")]:
        for parse_all in (True, False):
            got, ranges, route = ia.parse_container_view_by_index(blob, bad, (rect, m, 0), parse_all)
            assert route in (0, 1), what
            if parse_all:                                           # a hint only: the host's whole-frame verdict on the index
                assert route == ia.parse_container_by_index(blob, bad)[1], what
            if route == 1 or parse_all:
                assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges), (what, parse_all)
            refused += route
    assert refused >= 8


def test_an_index_whose_header_is_wrong_takes_route_one(ia):
    """what the host's check of the index against the container must refuse, whatever the window: the magic, the version, the
    container's size, its geometry, K, the block size, the stream and checkpoint counts, and a blob cut short"""
    blob = view_cases.main()
    rect, m = region_cases.ACROSS_1024, 2
    want, want_ranges = view_cases.expected_parse(blob, rect, m, region_cases.K)
    for version in (1, 2):
        index = ia.container_index(blob, 32, expanded=version == 2)
        bad = []
        for what, byte in (("magic", 0), ("version", 4), ("container bytes", 16), ("width", 24), ("height", 28), ("K", 32), ("block size", 36),
                           ("streams", 40), ("checkpoints", 48)):
            for bit in (0, 2):
                c = bytearray(index)
                c[byte] ^= 1 << bit
                bad.append((f"{what} bit {bit}", bytes(c)))
        bad += [(f"cut to {len(index) * k // 16}", index[:len(index) * k // 16]) for k in range(16)]
        for what, x in bad:
            for parse_all in (False, True):
                got, ranges, route = ia.parse_container_view_by_index(blob, x, (rect, m, 0), parse_all)
                assert route == 1, (version, what, parse_all)
                assert np.array_equal(got, want) and np.array_equal(ranges, want_ranges), (version, what, parse_all)


def test_streams_never_read(ia):
    """a container damaged only in a stream the view cuts away still yields its parse; with "parse all" the definition's answer"""
    blob, k = view_cases.main(), region_cases.K
    index = ia.container_index(blob, 32)
    damaged = view_cases.flip_in_stream(blob, index, 2 * k)
    assert damaged != blob
    want, want_ranges = view_cases.expected_parse(blob, view_cases.WHOLE, 2, k)
    got, ranges, route = ia.parse_container_view_by_index(damaged, index, (view_cases.WHOLE, 2, 0))
    assert route == 0 and np.array_equal(got, want) and np.array_equal(ranges, want_ranges)
    try:
        cut = ia.truncate_container(damaged, 2)
    except ia.MpcError as e:
        with pytest.raises(ia.MpcError) as mine:
            ia.parse_container_view_by_index(damaged, index, (view_cases.WHOLE, 2, 0), True)
        assert (mine.value.status, str(mine.value)) == (e.status, str(e))
    else:
        assert cut == ia.truncate_container(blob, 2)
        got, ranges, route = ia.parse_container_view_by_index(damaged, index, (view_cases.WHOLE, 2, 0), True)
        assert route in (0, 1) and np.array_equal(got, want) and np.array_equal(ranges, want_ranges)


def test_argument_errors(ia):
    blob = view_cases.main()
    index = ia.container_index(blob, 32)
    w, h = region_cases.W, region_cases.H
    bad = [((0, 0, 8, 8), -1, 0), ((0, 0, 8, 8), 0, 4), ((0, 0, 8, 8), 0, -1), ((1, 0, 8, 8), 0, 1), ((0, 2, 8, 8), 0, 2), ((4, 4, 8, 8), 0, 3),
           ((0, 0, 0, 5), 0, 0), ((0, 0, w + 1, h), 0, 0), ((w, 0, 1, 1), 0, 0), ((0, 8, 0, 0), 0, 0)]
    for view in bad:
        with pytest.raises(ia.MpcError) as e:
            ia.parse_container_view_by_index(blob, index, view)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, view
    with pytest.raises(ia.MpcError) as e:
        ia.parse_container_view_by_index(blob[:len(blob) // 2], index, (view_cases.WHOLE, 1, 0))
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid input data")
    ia.parse_container_view_by_index(blob, index, ((4, 4, 8, 8), 0, 2))       # an origin on the reduction's grid


def test_the_reduction_in_numpy(ia):
    """view_cases.reduce against the definition, pixel by pixel, on a ragged rectangle"""
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (11, 13, 3)).astype(np.uint8)
    for s in view_cases.SCALES:
        c = 1 << s
        got = view_cases.reduce(px, s)
        assert got.shape == (-(-11 // c), -(-13 // c), 3)
        for j in range(got.shape[0]):
            for i in range(got.shape[1]):
                cell = px[j * c:(j + 1) * c, i * c:(i + 1) * c].reshape(-1, 3).astype(int)
                assert list(got[j, i]) == [(int(v) + len(cell) // 2) // len(cell) for v in cell.sum(axis=0)]
