"""Decoding a pixel rectangle of a frame through its seek index on the GPU (run with -m gpu): both entry points and both flags
against the crop of the whole frame's decode, the device's windowed parse against its definition on the host, the serial route's
crop where there is no usable index, and damaged inputs.  Every equality is exact."""
import numpy as np
import pytest

import parse_cases
import region_cases
from container_cases import corpus as _corpus
from region_cases import crop

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
    return ia.create_compression_context(region_cases.K, 8, region_cases.QUALITY, device=0)


@pytest.fixture(scope="module")
def encoded(ctx):
    """{interval: (container, index)} of the shared frame, from the indexed encoder"""
    return {interval: ctx.encode_images_indexed([region_cases.frame()], interval)[0] for interval in region_cases.INTERVALS}


def _host(frames):
    return [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in frames]


def _check_regions(ctx, blobs, indexes, rects, fulls, routes_want, flags=(False, True)):
    """both entry points, both flags: the exact crops and the routes"""
    want = [crop(full, rect) for full, rect in zip(fulls, rects)]
    for parse_all in flags:
        for call in (ctx.decode_regions, ctx.decode_regions_device):
            frames, routes = call(blobs, indexes, rects, parse_all)
            assert routes == routes_want, (call.__name__, parse_all, routes)
            for n, (got, exp) in enumerate(zip(_host(frames), want)):
                assert got.shape == exp.shape, (call.__name__, parse_all, n, rects[n])
                assert np.array_equal(got, exp), (call.__name__, parse_all, n, rects[n])


@pytest.mark.parametrize("interval", region_cases.INTERVALS)
def test_every_rectangle_of_the_frame(ia, ctx, encoded, interval):
    blob, index = encoded[interval]
    assert index == ia.container_index(blob, interval)
    full = _host(ctx.decode_images([blob]))[0]
    rects = list(region_cases.RECTS)
    n = len(rects)
    _check_regions(ctx, [blob] * n, [index] * n, rects, [full] * n, [0] * n)
    for rect in rects:                                              # one frame a call as well: the calling thread's own path
        _check_regions(ctx, [blob], [index], [rect], [full], [0], flags=(False,))


@pytest.mark.parametrize("interval", region_cases.INTERVALS)
def test_window_parse_on_the_device_is_the_hosts(ia, ctx, encoded, interval):
    blob, index = encoded[interval]
    for rect in region_cases.RECTS:
        for parse_all in (False, True):
            host, host_ranges, host_route = ia.parse_container_window_by_index(blob, index, rect, parse_all)
            got, ranges, route = ctx.parse_container_window_device(blob, index, rect, parse_all)
            what = (interval, rect, parse_all)
            assert (route, host_route) == (0, 0), what
            assert np.array_equal(ranges, host_ranges), what
            assert got.shape == host.shape and np.array_equal(got, host), what


def test_float_flavour(ia, oracle, encoded):
    blob, index = encoded[32]
    fast = ia.create_compression_context(region_cases.K, 8, region_cases.QUALITY, device=0).set_fast(True)
    full = oracle.decode_image_fast(blob)
    rects = list(region_cases.RECTS)
    n = len(rects)
    _check_regions(fast, [blob] * n, [index] * n, rects, [full] * n, [0] * n)
    fast.close()


def test_a_context_of_another_k(ia, ctx, encoded):
    blob, index = encoded[100]
    other = ia.create_compression_context(3, 8, 6.0, device=0)
    assert other.K == 3 and ia.container_info(blob)[2] == 8
    full = _host(ctx.decode_images([blob]))[0]
    rects = list(region_cases.RECTS)
    n = len(rects)
    _check_regions(other, [blob] * n, [index] * n, rects, [full] * n, [0] * n)
    other.close()


def test_eight_gather_blocks(ia, oracle):
    """1003x517, K = 32: 126 x 65 = 8190 tiles"""
    ctx32 = ia.create_compression_context(32, 8, 3.5, device=0)
    blob, index = ctx32.encode_images_indexed([oracle.synth_frame(1003, 517, 103)], 100)[0]
    full = _host(ctx32.decode_images([blob]))[0]
    rects = [(0, 0, 1003, 517), (500, 250, 131, 77), (995, 3, 8, 514)]
    _check_regions(ctx32, [blob] * 3, [index] * 3, rects, [full] * 3, [0] * 3)
    for rect in rects:
        host, host_ranges, host_route = ia.parse_container_window_by_index(blob, index, rect)
        got, ranges, route = ctx32.parse_container_window_device(blob, index, rect)
        assert (route, host_route) == (0, 0) and np.array_equal(ranges, host_ranges) and np.array_equal(got, host), rect
    ctx32.close()


def test_tiny_frames(ia, ctx, oracle):
    for w, h in ((8, 8), (16, 8)):
        blob, index = ctx.encode_images_indexed([oracle.synth_frame(w, h, 5)], 32)[0]
        full = _host(ctx.decode_images([blob]))[0]
        rects = [(0, 0, w, h), (w - 1, 7, 1, 1), (3, 2, 4, 5), (w - 8, 0, 8, 8)]
        n = len(rects)
        _check_regions(ctx, [blob] * n, [index] * n, rects, [full] * n, [0] * n)


def test_route_one(ia, ctx, encoded):
    """no index, an index that says "serial only", an index that is none: the whole frame by the serial route, cropped"""
    blob, index = encoded[32]
    full = _host(ctx.decode_images([blob]))[0]
    serial_only = bytearray(index)
    serial_only[12] |= 1                                            # the flags word; the checkpoints stay, which no such index has
    assert ia.index_info(ia.container_index(blob, 32))["serial_only"] is False
    rects = [region_cases.ACROSS_1024, (0, 0, region_cases.W, region_cases.H), (260, 276, 1, 1), (5, 3, 50, 70)]
    indexes = [None, bytes(serial_only), b"not an index", index]
    _check_regions(ctx, [blob] * 4, indexes, rects, [full] * 4, [1, 1, 1, 0])


def test_a_sequence_with_differing_rectangles(ia, ctx, oracle):
    real = [b for _, b in parse_cases.real(oracle)]
    assert len(real) > 6                                            # more frames than decode slots
    fulls = _host(ctx.decode_images(real))
    rng = np.random.default_rng(20250307)
    rects = []
    for b in real:
        w, h, _, _ = ia.container_info(b)
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        rects.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
    indexes = [ia.container_index(b, 32) for b in real]
    _check_regions(ctx, real, indexes, rects, fulls, [0] * len(real))
    indexes[4] = None
    _check_regions(ctx, real, indexes, rects, fulls, [0] * 4 + [1] + [0] * (len(real) - 5))


def test_capacity_and_guard_band(ia, ctx, encoded):
    import torch
    blob, index = encoded[32]
    full = _host(ctx.decode_images([blob]))[0]
    for rect, idx in ((region_cases.ACROSS_1024, index), ((5, 3, 50, 70), index), ((5, 3, 50, 70), None)):
        need = 3 * rect[2] * rect[3]
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        frames, routes = ctx.decode_regions_device([blob], [idx], [rect], out=[buf[:need]])
        assert routes == [0 if idx else 1]
        assert np.array_equal(_host(frames)[0], crop(full, rect))
        assert bool((buf[need:] == 0xA5).all()), rect
        with pytest.raises(ia.MpcError) as e:
            ctx.decode_regions_device([blob, blob], [idx, idx], [rect, rect], out=[buf[:need], buf[need:2 * need - 1]])
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "frame 1: capacity" in str(e.value)


def test_rectangles_are_checked_before_anything_runs(ia, ctx, encoded):
    blob, index = encoded[32]
    w, h = region_cases.W, region_cases.H
    for rect in ((0, 0, 0, 5), (3, 3, 2, -1), (-1, 0, 4, 4), (w, 0, 1, 1), (w - 3, 0, 4, 1), (0, h - 3, 1, 4), (0, 0, w, h + 1)):
        for call in (ctx.decode_regions, ctx.decode_regions_device):
            with pytest.raises(ia.MpcError) as e:
                call([blob, blob], [index, index], [(0, 0, 8, 8), rect])
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "frame 1: rectangle" in str(e.value), rect
    frames, routes = ctx.decode_regions([blob], [index], [(0, 0, 8, 8)])
    assert routes == [0]


def test_damaged_indexes_with_parse_all(ia, ctx, oracle, encoded):
    """the index is a hint only: the exact crop whatever it holds, and the context still decodes afterwards"""
    blob, index = encoded[32]
    full = _host(ctx.decode_images([blob]))[0]
    other = ctx.encode_images_indexed([oracle.synth_frame(region_cases.W, region_cases.H, 778)], 32)[0][1]
    damaged = parse_cases.damaged_indexes(index, other, 0)
    rect = region_cases.ACROSS_1024
    by_route = [0, 0]
    for k in range(0, len(damaged), 8):
        some = damaged[k:k + 8]
        call = ctx.decode_regions if (k // 8) % 2 == 0 else ctx.decode_regions_device
        frames, routes = call([blob] * len(some), [bad for _, bad in some], [rect] * len(some), True)
        assert set(routes) <= {0, 1}
        for got in _host(frames):
            assert np.array_equal(got, crop(full, rect))
        for route in routes:
            by_route[route] += 1
    assert by_route[1] >= 1, by_route
    for what, bad in damaged[:24]:                                  # the device refuses what the host's definition refuses
        host, _, host_route = ia.parse_container_window_by_index(blob, bad, rect, True)
        got, _, route = ctx.parse_container_window_device(blob, bad, rect, True)
        assert route == host_route and np.array_equal(got, host), what
    _check_regions(ctx, [blob], [index], [rect], [full], [0])


@pytest.mark.parametrize("which", range(8))
def test_damaged_containers_with_parse_all(ia, ctx, oracle, which):
    """the status and text of decode_images, or the exact crop"""
    n, blob, xs = list(_corpus(oracle))[which]
    index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
    w, h, _, _ = ia.container_info(blob)
    rect = (w // 3, h // 4, w - w // 3, h // 2 + 1)
    refused = 0
    for k, x in enumerate(xs):
        call = ctx.decode_regions if k % 2 == 0 else ctx.decode_regions_device
        try:
            full = _host(ctx.decode_images([x]))[0]
        except ia.MpcError as e:
            try:
                call([x], [index], [rect], True)
            except ia.MpcError as mine:
                if mine.status == ia.api.MPC_ERR_ARGUMENT and "rectangle" in str(mine):
                    info = ia.container_info(x)                     # a damaged header: the rectangle is outside ITS frame
                    assert not (rect[0] + rect[2] <= info[0] and rect[1] + rect[3] <= info[1]), k
                else:
                    assert (mine.status, str(mine)) == (e.status, str(e)), k
            else:                                                   # a record outside its dictionary, in a tile the window does not hold:
                assert str(e).endswith("Invalid bitstream"), k      # that verdict speaks for the window's tiles only
            refused += 1
            continue
        if full.shape[:2] != (h, w):                                # a damaged header that still decodes: another frame
            continue
        frames, routes = call([x], [index], [rect], True)
        assert routes[0] in (0, 1) and np.array_equal(_host(frames)[0], crop(full, rect)), k
    assert refused > 10
    frames, routes = ctx.decode_regions([blob], [index], [rect], True)
    assert routes == [0] and np.array_equal(frames[0], crop(oracle.decode_image(blob), rect))
