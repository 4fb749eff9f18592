"""Decoding with a seek index on the GPU (run with -m gpu): the device parse (mp_parse.hip) against the chunked parse on the host
and the serial parse, sequences with indexes against sequences without, and the rule that an index is a hint only: pixels,
statuses and error texts are those of the serial route whatever an index holds.  Every equality is exact."""
import numpy as np
import pytest

import parse_cases
from container_cases import corpus as _corpus
from parse_cases import INTERVALS

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
    return ia.create_compression_context(8, 8, 3.5, device=0)


@pytest.fixture(scope="module")
def real(oracle):
    return parse_cases.real(oracle)


def _same_symbols(got, blob, what):
    want, sizes = parse_cases.serial(blob)
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        off = np.cumsum([0] + sizes)
        stream = int(np.searchsorted(off, at, side="right")) - 1
        raise AssertionError(f"{what}: first difference at symbol {at}: stream {stream - 1} (-1 = lengths) position {at - off[stream]} of "
                             f"{sizes[stream]}: {got[at]} != {want[at]}")


def _host(frames):
    return [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in frames]


def _equal_frames(got, want):
    assert len(got) == len(want)
    for n, (a, b) in enumerate(zip(_host(got), want)):
        assert a.shape == b.shape, n
        assert np.array_equal(a, b), n


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_parse_entry(ia, ctx, name):
    parse_cases.check_coverage(ia)
    blob = parse_cases.synthetic()[name]
    for interval in INTERVALS:
        index = ia.container_index(blob, interval)
        host, route = ia.parse_container_by_index(blob, index)
        assert route == 0
        _same_symbols(host, blob, f"{name} at {interval} on the host")
        got, route = ctx.parse_container_device(blob, index)
        assert route == 0, (name, interval)
        _same_symbols(got, blob, f"{name} at {interval} on the device")


def test_sequences(ia, ctx, oracle, real):
    blobs = [b for _, b in real]                                    # A - D hold random records: they parse, they do not reconstruct
    order = np.random.default_rng(20250306).permutation(len(blobs))
    blobs = [blobs[i] for i in order]
    assert len(blobs) > 6                                           # more frames than decode slots
    want = _host(ctx.decode_images(blobs))
    for interval in (0, 100):
        indexes = [ia.container_index(b, interval) for b in blobs]
        frames, routes = ctx.decode_images_indexed(blobs, indexes)
        assert routes == [0] * len(blobs)
        _equal_frames(frames, want)
        frames, routes = ctx.decode_images_indexed_device(blobs, indexes)
        assert routes == [0] * len(blobs)
        _equal_frames(frames, want)
    # a frame without an index in the middle
    indexes[5] = None
    for call in (ctx.decode_images_indexed, ctx.decode_images_indexed_device):
        frames, routes = call(blobs, indexes)
        assert routes == [0] * 5 + [1] + [0] * (len(blobs) - 6)
        _equal_frames(frames, want)
    frames, routes = ctx.decode_images_indexed(blobs, [None] * len(blobs))
    assert routes == [1] * len(blobs)
    _equal_frames(frames, want)
    small = real[2][1]
    frames, routes = ctx.decode_images_indexed([small], [ia.container_index(small)])
    assert routes == [0] and np.array_equal(frames[0], oracle.decode_image(small))


def test_golden_frame(ia):
    mn = parse_cases.golden_mn()
    ctx32 = ia.create_compression_context(32, 8, 3.5, device=0)
    want = _host(ctx32.decode_images([mn]))
    index = ia.container_index(mn)
    got, route = ctx32.parse_container_device(mn, index)
    assert route == 0
    _same_symbols(got, mn, "the golden frame on the device")
    for call in (ctx32.decode_images_indexed, ctx32.decode_images_indexed_device):
        frames, routes = call([mn], [index])
        assert routes == [0]
        _equal_frames(frames, want)
    ctx32.close()


def _twins(ia, oracle, cases):
    others = dict(list(parse_cases.synthetic(1).items()) + parse_cases.real(oracle, seed=150))
    for n, (name, blob) in enumerate(cases):
        index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
        other = ia.container_index(others[name], parse_cases.EDGE_INTERVAL) if name in others else ia.container_index(blob, 64)
        yield name, blob, parse_cases.damaged_indexes(index, other, n)


def test_the_index_is_only_a_hint(ia, ctx, oracle, real):
    """the damaged indexes of the host test: flips inside the checkpoint tables pass the host's checks and reach the device's"""
    on_device = 0
    # A - D hold random records (they parse, they do not reconstruct): the parse entry alone
    for name, blob, damaged in _twins(ia, oracle, list(parse_cases.synthetic().items())):
        symbols, _ = parse_cases.serial(blob)
        refused = 0
        for what, bad in damaged:
            got, route = ctx.parse_container_device(blob, bad)
            assert np.array_equal(got, symbols), (name, what)
            assert route == ia.parse_container_by_index(blob, bad)[1], (name, what)
            refused += route
        assert refused >= 1, name
    ctx32 = ia.create_compression_context(32, 8, 3.5, device=0)
    for name, blob, damaged in _twins(ia, oracle, real + [("mn", parse_cases.golden_mn())]):
        ctx = ctx32 if name == "mn" else ctx
        want = _host(ctx.decode_images([blob]))
        symbols, _ = parse_cases.serial(blob)
        by_route = [0, 0]
        for k in range(0, len(damaged), 8):
            some = damaged[k:k + 8]
            call = ctx.decode_images_indexed if (k // 8) % 2 == 0 else ctx.decode_images_indexed_device
            frames, routes = call([blob] * len(some), [bad for _, bad in some])
            assert set(routes) <= {0, 1}, name
            _equal_frames(frames, want * len(some))
            for route in routes:
                by_route[route] += 1
        for what, bad in damaged[:24]:
            got, route = ctx.parse_container_device(blob, bad)
            host, host_route = ia.parse_container_by_index(blob, bad)
            assert np.array_equal(got, symbols) and np.array_equal(host, symbols), (name, what)
            # the host's chunk decoder and the device's refuse the same indexes
            assert route == host_route, (name, what)
            on_device += host_route == 1
        assert by_route[1] >= 1, (name, by_route)
        _equal_frames(ctx.decode_images_indexed([blob], [ia.container_index(blob)])[0], want)     # and the context still decodes
    assert on_device >= 1
    ctx32.close()


@pytest.mark.parametrize("which", range(8))
def test_same_refusals(ia, ctx, oracle, which):
    """the 768 damaged containers with the undamaged container's index: status and text are decode_images's"""
    n, blob, xs = list(_corpus(oracle))[which]
    index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
    want = oracle.decode_image(blob)
    refused = 0
    for k, x in enumerate(xs):
        pairs = ((ctx.decode_images, ctx.decode_images_indexed), (ctx.decode_images_device, ctx.decode_images_indexed_device))
        for plain, indexed in pairs:
            try:
                expect = _host(plain([x]))
            except ia.MpcError as e:
                with pytest.raises(ia.MpcError) as mine:
                    indexed([x], [index])
                assert (mine.value.status, str(mine.value)) == (e.status, str(e)), k
                refused += 1
                continue
            frames, routes = indexed([x], [index])
            assert routes[0] in (0, 1)
            _equal_frames(frames, expect)
        if k % 32 == 31:
            frames, routes = ctx.decode_images_indexed([blob], [index])
            assert routes == [0] and np.array_equal(frames[0], want)
    assert refused > 10
    frames, routes = ctx.decode_images_indexed_device([blob], [index])
    assert routes == [0] and np.array_equal(_host(frames)[0], want)


def test_other_contexts(ia, oracle, real):
    """the float flavour, and containers whose K and quantiser tables are not the context's"""
    blobs = [b for _, b in real]
    indexes = [ia.container_index(b) for b in blobs]
    fast = ia.create_compression_context(8, 8, 3.5, device=0).set_fast(True)
    want = [oracle.decode_image_fast(b) for b in blobs]
    _equal_frames(fast.decode_images(blobs), want)
    for call in (fast.decode_images_indexed, fast.decode_images_indexed_device):
        frames, routes = call(blobs, indexes)
        assert routes == [0] * len(blobs)
        _equal_frames(frames, want)
    fast.close()
    other = ia.create_compression_context(3, 8, 6.0, device=0)
    assert {ia.container_info(b)[2] for b in blobs} - {3} and other.K == 3
    want = _host(other.decode_images(blobs))
    frames, routes = other.decode_images_indexed(blobs, indexes)
    assert routes == [0] * len(blobs)
    _equal_frames(frames, want)
    other.close()
