"""The unpack, the window cut and the run-length plan beyond one trip of 64 blocks, on the GPU (run with -m gpu): the two hand-made
frames of trip_cases through the whole unpack, the whole parse, the windowed parse at every named rectangle and interval, exit
entries damaged behind block 64, and the entropy stage with its version-2 index.  The expectation is trip_cases' numpy and the
oracle's writeCompressed; every equality is exact.  No pixels are decoded: the symbols are no valid records."""
import numpy as np
import pytest

import trip_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def ctx(ia):
    """{frame: context of the frame's K}, one of each for the whole module"""
    made = {name: ia.create_compression_context(K, 8, 3.5, device=0) for name, (_, _, K) in tc.FRAMES.items()}
    yield made
    for c in made.values():
        c.close()


def _sizes(name):
    return [len(s) for s in tc.frame(name)["want"]]


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("name", tc.FRAMES)
def test_whole_unpack(ia, ctx, name, force):
    f = tc.frame(name)
    coded, packed = tc.coded_form(f["as_coded"], force)
    assert all(np.array_equal(c, ia.run_length_encode(s)) for c, s, p in zip(coded, f["as_coded"], packed) if p)
    assert sum(packed) == sum(len(s) > (0 if force else 1) for s in f["as_coded"])
    got = ctx[name].unpack_symbol_streams_device(coded, packed, _sizes(name))
    assert tc.first_difference(got, tc.expected_whole(name), _sizes(name)) is None, tc.first_difference(got, tc.expected_whole(name), _sizes(name))


@pytest.mark.parametrize("name", tc.FRAMES)
def test_whole_parse_route(ia, ctx, name):
    blob = tc.container(name)
    want, host_route = ia.parse_container_by_index(blob, tc.index(name, 128))
    assert host_route == 0 and np.array_equal(want, tc.expected_serial(name))
    for index in (ia.container_index(blob, 128), tc.index(name, 128), tc.index(name, 32)):
        got, route = ctx[name].parse_container_device(blob, index)
        assert route == 0
        assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("interval", tc.INTERVALS)
@pytest.mark.parametrize("rect_name", tc.RECTS)
def test_window_cut(ia, ctx, rect_name, interval):
    """a route of 1 is a failure: it is what a lost carry gives (stream_ok false, the host answers), and the symbols alone hide it"""
    name, rect, _ = tc.RECTS[rect_name]
    blob, v2 = tc.container(name), tc.index(name, interval)
    want, want_ranges = tc.expected_window(name, rect)
    sizes = tc.window_sizes(name, want_ranges)
    for parse_all in (False, True):
        got, ranges, route = ctx[name].parse_container_window_device(blob, v2, rect, parse_all)
        assert route == 0, parse_all
        assert np.array_equal(ranges, want_ranges), parse_all
        assert tc.first_difference(got, want, sizes, True) is None, (parse_all, tc.first_difference(got, want, sizes, True))
        chunks, chunks_route = ctx[name].window_chunks_device(blob, v2, rect, parse_all)
        host_chunks, host_chunks_route = ia.window_chunks_by_index(blob, v2, rect, parse_all)
        assert (chunks_route, host_chunks_route) == (0, 0) and np.array_equal(chunks, host_chunks), parse_all


def test_exit_checks_at_a_far_block(ia, ctx):
    """one bit of out, prev, state and dc of entry c1 of streams that leave behind block 64: the host's route, the expectation
    either way, and the undamaged index afterwards"""
    name, rect, _ = tc.RECTS[tc.FLIP_RECT]
    blob = tc.container(name)
    want, _ = tc.expected_window(name, rect)
    refused = 0
    for what, bad in tc.far_exit_flips(ia):
        _, _, host_route = ia.parse_container_window_by_index(blob, bad, rect)
        got, _, route = ctx[name].parse_container_window_device(blob, bad, rect)
        assert route == host_route, what
        assert got.shape == want.shape and np.array_equal(got, want), what
        refused += route
    assert refused >= 10, refused
    got, _, route = ctx[name].parse_container_window_device(blob, tc.index(name, tc.FLIP_INTERVAL), rect)
    assert route == 0 and np.array_equal(got, want)


def test_encode_direction(ia, ctx, oracle):
    """the entropy stage on B: a run across symbol 262 144 of stream 0, a run boundary exactly there in every other stream"""
    f = tc.frame("B")
    want = bytes(oracle.write_compressed(dict(W=f["W"], H=f["H"], K=f["K"], bs=8, quant=f["quant"], lengths=f["counts"], codes=f["as_held"])))
    assert want == tc.container("B")
    for attempt in range(2):                       # twice: the second call finds the tables the first one left behind
        got, route = ctx["B"].code_symbol_streams_device(f["W"], f["H"], f["counts"], f["as_coded"], quant=f["quant"])
        assert route == 0, "the device route was not taken"
        assert len(got) == len(want), (attempt, len(got), len(want))
        assert got == want, f"first differing byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)} (call {attempt})"
    for interval in (100, 32):
        got, index, route = ctx["B"].code_symbol_streams_device_indexed(f["W"], f["H"], f["counts"], f["as_coded"], interval, quant=f["quant"],
                                                                        expanded=True)
        assert route == 0 and got == want, interval
        assert index == tc.index("B", interval), interval


def test_encode_direction_of_a(ia, ctx):
    f = tc.frame("A")
    got, index, route = ctx["A"].code_symbol_streams_device_indexed(f["W"], f["H"], f["counts"], f["as_coded"], 100, quant=f["quant"], expanded=True)
    assert route == 0 and got == tc.container("A") and index == tc.index("A", 100)


def test_usable_afterwards(ia, ctx, oracle):
    """after everything above each context still decodes a small oracle container exactly"""
    rgb = oracle.synth_frame(64, 40, 5)
    for name, (_, _, K) in tc.FRAMES.items():
        blob = bytes(oracle.OracleContext(K, 8, 3.5).encode_image(rgb))
        got = ctx[name].decode_images([blob])[0]
        got = np.asarray(got.cpu()) if hasattr(got, "cpu") else np.asarray(got)
        assert np.array_equal(got, oracle.decode_image(blob))
