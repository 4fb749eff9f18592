"""The seek index from a bit scan on the GPU (run with -m gpu): mp_scan.hip's step table, segment maps, chain and walk against the
serial builder, and the decode of frames that come without an index through it.  For every input the status, the error text and
the blob are mpc_container_index2's, and pixels, statuses and error texts are decode_images's; route 0 is required wherever the
serially built index is one the chunked parse uses.  Every equality is exact."""
import numpy as np
import pytest

import parse_cases
from container_cases import corpus as _corpus
from parse_cases import INTERVALS
from test_index_scan_host import CORPUS_ROUTE_0

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


def _host(frames):
    return [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in frames]


def _equal_frames(got, want):
    assert len(got) == len(want)
    for n, (a, b) in enumerate(zip(_host(got), want)):
        assert a.shape == b.shape, n
        assert np.array_equal(a, b), n


def test_index_entry(ia, ctx, real):
    for name, blob in list(parse_cases.synthetic().items()) + real:
        for interval in INTERVALS:
            for flags in (0, ia.api.MPC_INDEX_EXPANDED):
                got, route = ctx.container_index_device(blob, interval, flags)
                assert route == 0, (name, interval, flags)
                assert got == ia.container_index2(blob, interval, flags), (name, interval, flags)


@pytest.mark.parametrize("sizes", [(32, 64), (256, 1024), (4096, 8192)])
def test_small_segments_and_windows(ia, ctx, sizes):
    """the smallest inputs on which a chain crosses windows (all three), a code jumps segments (D's unary runs; C's 20-bit codes
    against 32-bit segments) and a table is deeper than the window table (C).  Segments of 4096 bits take the segment kernel that
    works in global memory; up to 256 bits the one that works in LDS"""
    for name in ("A", "C", "D"):
        blob = parse_cases.synthetic()[name]
        for interval in INTERVALS:
            got, route = ctx.debug_container_index_device(blob, interval, *sizes)
            assert route == 0, (name, interval)
            assert got == ia.container_index(blob, interval), (name, interval)


def test_golden_frame(ia):
    mn = parse_cases.golden_mn()
    ctx32 = ia.create_compression_context(32, 8, 3.5, device=0)
    got, route = ctx32.container_index_device(mn)
    assert route == 0 and got == ia.container_index(mn)
    want = _host(ctx32.decode_images([mn]))
    for call in (ctx32.decode_images_scan, ctx32.decode_images_scan_device):
        frames, routes = call([mn])
        assert routes == [0]
        _equal_frames(frames, want)
    ctx32.close()


def test_sequences(ia, ctx, real):
    """more frames than decode slots; A - D hold random records (they parse, they do not reconstruct), so they go through the index
    entry above and the frames here are E's, each twice"""
    blobs = [b for _, b in real] + [b for _, b in real[:4]]
    order = np.random.default_rng(20250912).permutation(len(blobs))
    blobs = [blobs[i] for i in order]
    assert len(blobs) == 12
    want = _host(ctx.decode_images(blobs))
    for again in range(2):                                          # the second call reuses the slots' grown scratch
        for call in (ctx.decode_images_scan, ctx.decode_images_scan_device):
            frames, routes = call(blobs)
            assert routes == [0] * len(blobs), again
            _equal_frames(frames, want)
            frames, routes, indexes = call(blobs, keep_indexes=True)
            assert routes == [0] * len(blobs), again
            _equal_frames(frames, want)
            assert indexes == [ia.container_index(b) for b in blobs], again


@pytest.mark.parametrize("which", range(8))
def test_damaged_containers(ia, ctx, oracle, which):
    """the 768 damaged containers: the index entry gives the serial builder's status, text and blob, the decode decode_images's
    pixels or error text; route 0 under the host test's rule.  The count over all eight cases is the host test's (CORPUS_ROUTE_0);
    here every case checks its own against the rule"""
    n, blob, xs = list(_corpus(oracle))[which]
    scanned = must = 0
    for k, x in enumerate(xs):
        flags = k % 2
        try:
            want = ia.container_index2(x, parse_cases.EDGE_INTERVAL, flags)
        except ia.MpcError as e:
            with pytest.raises(ia.MpcError) as mine:
                ctx.container_index_device(x, parse_cases.EDGE_INTERVAL, flags)
            assert (mine.value.status, str(mine.value)) == (e.status, str(e)), k
            want = None
        if want is not None:
            got, route = ctx.container_index_device(x, parse_cases.EDGE_INTERVAL, flags)
            assert got == want, k
            if ia.parse_container_by_index(x, want)[1] == 0:
                must += 1
                assert route == 0, k
            scanned += route == 0
        try:
            expect = _host(ctx.decode_images([x]))
        except ia.MpcError as e:
            with pytest.raises(ia.MpcError) as mine:
                ctx.decode_images_scan([x])
            assert (mine.value.status, str(mine.value)) == (e.status, str(e)), k
            continue
        frames, routes = ctx.decode_images_scan([x])
        assert routes[0] in (0, 1)
        _equal_frames(frames, expect)
    assert scanned == must
    _COUNTS[which] = scanned
    if len(_COUNTS) == 8:
        assert sum(_COUNTS.values()) == CORPUS_ROUTE_0
    frames, routes = ctx.decode_images_scan([blob])
    assert routes == [0] and np.array_equal(frames[0], oracle.decode_image(blob))


_COUNTS = {}
