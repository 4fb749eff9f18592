"""Views on the GPU (run with -m gpu): the first `steps` records of every tile-channel, reduced 1/2/4/8x, of a frame or a
rectangle of it, through both entry points and both routes, against the ORACLE's decode of the truncated container cropped and
reduced in numpy (view_cases); the device's parse of a view against its definition on the host; streams a view never reads; the
dictionary built from the first `steps` choices; argument errors.  Every equality is exact."""
import numpy as np
import pytest

import parse_cases
import region_cases
import view_cases
from view_cases import WHOLE, expected_view

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
def inputs(ia, oracle):
    """{name: (container, {version: index}, steps)}: both index versions at interval 32"""
    out = {}
    for name, blob, steps in (("main", view_cases.main(), view_cases.STEPS), ("small", view_cases.small(), view_cases.SMALL_STEPS)):
        out[name] = (blob, {1: ia.container_index(blob, 32), 2: ia.container_index(blob, 32, expanded=True)}, steps)
    return out


def _host(frames):
    return [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in frames]


def _check_views(ctx, blobs, indexes, views, routes_want, parse_all=False, fast=False, calls=None):
    """both entry points: the exact pixels, the output's shape and the routes"""
    want = [expected_view(blob, view, fast) for blob, view in zip(blobs, views)]
    for call in calls or (ctx.decode_views, ctx.decode_views_device):
        frames, routes = call(blobs, indexes, views, parse_all)
        assert routes == routes_want, (call.__name__, routes)
        for n, (got, exp) in enumerate(zip(_host(frames), want)):
            assert got.shape == exp.shape, (call.__name__, n, views[n], got.shape, exp.shape)
            assert np.array_equal(got, exp), (call.__name__, n, views[n])


@pytest.mark.parametrize("name", ("main", "small"))
@pytest.mark.parametrize("version", (1, 2))
def test_whole_frames(ia, ctx, inputs, name, version):
    blob, indexes, steps = inputs[name]
    views = [(WHOLE, m, s) for m in steps for s in view_cases.SCALES]
    n = len(views)
    _check_views(ctx, [blob] * n, [indexes[version]] * n, views, [0] * n)
    _check_views(ctx, [blob], [indexes[version]], [(WHOLE, 1, 3)], [0])     # one frame a call: the calling thread's own path
    full = _host(ctx.decode_images([blob]))[0]
    frames, routes = ctx.decode_views([blob], [indexes[version]], [(WHOLE, 0, 0)])
    assert routes == [0] and np.array_equal(frames[0], full)


@pytest.mark.parametrize("version", (1, 2))
def test_rectangles(ia, ctx, inputs, version):
    blob, indexes, _ = inputs["main"]
    for m in (0, 2):
        views = [(rect, m, s) for rect in view_cases.RECTS for s in view_cases.SCALES]
        n = len(views)
        _check_views(ctx, [blob] * n, [indexes[version]] * n, views, [0] * n)
        _check_views(ctx, [blob] * n, [indexes[version]] * n, views, [0] * n, parse_all=True, calls=(ctx.decode_views_device,))
    # an origin off the reduction's grid: at scale 0 the region of the truncated container, at scale 1 an argument error
    rect = view_cases.UNALIGNED
    cut = ia.truncate_container(blob, 2)
    want, _ = ctx.decode_regions([cut], [ia.container_index(cut, 32)], [rect])
    for call in (ctx.decode_views, ctx.decode_views_device):
        frames, routes = call([blob], [indexes[version]], [(rect, 2, 0)])
        assert routes == [0] and np.array_equal(_host(frames)[0], want[0])
        with pytest.raises(ia.MpcError) as e:
            call([blob, blob], [indexes[version]] * 2, [(WHOLE, 2, 1), (rect, 2, 1)])
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "frame 1: " in str(e.value)


def test_identity_with_the_region_decoder(ia, ctx, inputs):
    blob, indexes, _ = inputs["main"]
    rects = list(region_cases.RECTS)
    n = len(rects)
    want, _ = ctx.decode_regions([blob] * n, [indexes[2]] * n, rects)
    for call in (ctx.decode_views, ctx.decode_views_device):
        frames, routes = call([blob] * n, [indexes[2]] * n, [(rect, 0, 0) for rect in rects])
        assert routes == [0] * n
        for got, exp, rect in zip(_host(frames), want, rects):
            assert np.array_equal(got, exp), rect


def test_route_one(ia, ctx, oracle, inputs):
    """no index, an index that is none, damaged indexes: the serial parse, the same pixels"""
    blob, indexes, _ = inputs["main"]
    views = [(region_cases.ACROSS_1024, 2, 1), (WHOLE, 1, 3), ((256, 0, 5, 277), 3, 2), (WHOLE, 0, 0), (WHOLE, 9, 1)]
    _check_views(ctx, [blob] * 5, [None, b"not an index", None, None, indexes[1]], views, [1, 1, 1, 1, 0])
    small, small_indexes, _ = inputs["small"]
    _check_views(ctx, [small] * 3, [None] * 3, [(WHOLE, 5, 1), ((8, 8, 17, 9), 1, 2), (WHOLE, 40, 3)], [1] * 3)
    other = ia.container_index(bytes(oracle.OracleContext(region_cases.K, 8, region_cases.QUALITY).encode_image(
        oracle.synth_frame(region_cases.W, region_cases.H, 778))), 32)
    damaged = parse_cases.damaged_indexes(indexes[1], other, 0)
    view = (region_cases.ACROSS_1024, 2, 1)
    want = expected_view(blob, view)
    by_route = [0, 0]
    for k in range(0, len(damaged), 8):
        some = damaged[k:k + 8]
        call = ctx.decode_views if (k // 8) % 2 == 0 else ctx.decode_views_device
        frames, routes = call([blob] * len(some), [bad for _, bad in some], [view] * len(some), True)      # a hint only
        for got, route in zip(_host(frames), routes):
            assert route in (0, 1) and np.array_equal(got, want)
            by_route[route] += 1
        frames, routes = call([blob] * len(some), [bad for _, bad in some], [view] * len(some))
        for got, route, (what, _) in zip(_host(frames), routes, some):
            assert route in (0, 1), what
            if route == 1:
                assert np.array_equal(got, want), what
    assert by_route[1] >= 8, by_route
    # what the host's check of the index must refuse, whatever the window: route 1 outright, with or without "parse all"
    wrong = []
    for version in (1, 2):
        for byte in (0, 4, 16, 24, 32, 40, 48):                     # magic, version, container bytes, width, K, streams, checkpoints
            c = bytearray(indexes[version])
            c[byte] ^= 1
            wrong.append(bytes(c))
        wrong.append(indexes[version][:len(indexes[version]) // 2])
    n = len(wrong)
    for parse_all in (False, True):
        _check_views(ctx, [blob] * n, wrong, [view] * n, [1] * n, parse_all=parse_all)
    _check_views(ctx, [blob], [indexes[1]], [view], [0])


def test_float_flavour(ia, inputs):
    fast = ia.create_compression_context(region_cases.K, 8, region_cases.QUALITY, device=0).set_fast(True)
    blob, indexes, _ = inputs["main"]
    views = [(rect, m, s) for rect in (WHOLE,) + view_cases.RECTS for m in (1, 8) for s in (0, 3)]
    n = len(views)
    for version in (1, 2):
        _check_views(fast, [blob] * n, [indexes[version]] * n, views, [0] * n, fast=True)
    _check_views(fast, [blob] * n, [None] * n, views, [1] * n, fast=True, calls=(fast.decode_views,))
    fast.close()


def test_streams_never_read(ia, ctx, oracle, inputs):
    """one bit flipped in the coefficients of the last step: a view of two steps never reads it; "parse all" answers as the
    definition does for the damaged bytes"""
    blob, indexes, _ = inputs["main"]
    k = region_cases.K
    damaged = view_cases.flip_in_stream(blob, indexes[1], 2 * k)
    views = [(WHOLE, 2, 0), (region_cases.ACROSS_1024, 2, 1), (WHOLE, 2, 3)]
    want = [expected_view(blob, view) for view in views]
    for version in (1, 2):
        for call in (ctx.decode_views, ctx.decode_views_device):
            frames, routes = call([damaged] * 3, [indexes[version]] * 3, views)
            assert routes == [0] * 3
            for got, exp in zip(_host(frames), want):
                assert np.array_equal(got, exp)
    try:
        cut = ia.truncate_container(damaged, 2)
    except ia.MpcError as e:
        definition = e
    else:
        definition = [view_cases.reduce(region_cases.crop(oracle.decode_image(cut), view_cases.resolve(v[0], region_cases.W, region_cases.H)), v[2])
                      for v in views]
    for call in (ctx.decode_views, ctx.decode_views_device):
        if isinstance(definition, ia.MpcError):
            with pytest.raises(ia.MpcError) as mine:
                call([damaged] * 3, [indexes[1]] * 3, views, True)
            assert mine.value.status == definition.status == ia.api.MPC_ERR_BITSTREAM
            assert str(mine.value).endswith("frame 0: Invalid input data") and str(definition).endswith("Invalid input data")
        else:
            frames, routes = call([damaged] * 3, [indexes[1]] * 3, views, True)
            assert set(routes) <= {0, 1}
            for got, exp in zip(_host(frames), definition):
                assert np.array_equal(got, exp)
    # the whole container, damaged there: what decode_images says of it, with or without an index
    try:
        full = _host(ctx.decode_images([damaged]))[0]
    except ia.MpcError as e:
        with pytest.raises(ia.MpcError) as mine:
            ctx.decode_views([damaged], [indexes[1]], [(WHOLE, 0, 0)])
        assert (mine.value.status, str(mine.value)) == (e.status, str(e))
    else:
        frames, routes = ctx.decode_views([damaged], [indexes[1]], [(WHOLE, 0, 0)])
        assert np.array_equal(frames[0], full)


@pytest.mark.parametrize("route", (0, 1))
def test_the_dictionary_is_built_from_the_first_steps(ia, ctx, oracle, route):
    for discriminating in (False, True):
        hand = view_cases.dictionary_case(ia, discriminating)
        index = ia.container_index(hand, 32) if route == 0 else None
        full = oracle.decode_image(hand)                            # the full list decodes
        for call in (ctx.decode_views, ctx.decode_views_device):
            for m in (1, 3, 0) + (() if discriminating else (2,)):
                frames, routes = call([hand], [index], [(WHOLE, m, 0)])
                want = full if m == 0 else oracle.decode_image(view_cases.truncated(hand, m))
                assert routes == [route] and np.array_equal(_host(frames)[0], want), (discriminating, m)
            if discriminating:
                with pytest.raises(ia.MpcError) as whole:             # the truncated container itself: row 573 is outside its dictionary
                    ctx.decode_images([ia.truncate_container(hand, 2)])
                for parse_all in (False, True):
                    with pytest.raises(ia.MpcError) as e:
                        call([hand], [index], [(WHOLE, 2, 0)], parse_all)
                    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("frame 0: Invalid bitstream")
                    assert (e.value.status, str(e.value)) == (whole.value.status, str(whole.value))
                frames, _ = call([hand], [index], [(WHOLE, 1, 3)])
                assert np.array_equal(_host(frames)[0], expected_view(hand, (WHOLE, 1, 3)))


def test_a_sequence_of_differing_views(ia, ctx, inputs):
    """eight frames, more than the decode slots: both inputs, differing views, one frame without an index"""
    main, main_indexes, _ = inputs["main"]
    small, small_indexes, _ = inputs["small"]
    blobs = [main, small, main, main, small, main, small, main]
    indexes = [main_indexes[1], small_indexes[2], main_indexes[2], None, small_indexes[1], main_indexes[2], small_indexes[2], main_indexes[1]]
    views = [(WHOLE, 1, 3), (WHOLE, 5, 0), (region_cases.ACROSS_1024, 3, 1), ((256, 0, 5, 277), 2, 2), ((8, 8, 17, 9), 40, 1), (WHOLE, 0, 2),
             (WHOLE, 1, 3), ((0, 272, 261, 5), 8, 0)]
    routes_want = [0, 0, 0, 1, 0, 0, 0, 0]
    _check_views(ctx, blobs, indexes, views, routes_want)
    for call in (ctx.decode_views, ctx.decode_views_device):
        together, _ = call(blobs, indexes, views)
        for n in range(len(blobs)):
            alone, routes = call([blobs[n]], [indexes[n]], [views[n]])
            assert routes == [routes_want[n]] and np.array_equal(_host(alone)[0], _host(together)[n]), n


def test_view_parse_on_the_device_is_the_hosts(ia, ctx, inputs):
    blob, _, _ = inputs["main"]
    small, _, _ = inputs["small"]
    matrix = [(blob, view_cases.PARSE_STEPS, view_cases.PARSE_RECTS), (small, (1, 5, 32, 0), (WHOLE, (8, 8, 17, 9)))]
    for container, steps, rects in matrix:
        for version in (1, 2):
            for interval in (32, 0):
                index = ia.container_index(container, interval, expanded=version == 2)
                for m in steps:
                    for rect in rects:
                        for parse_all in (False, True):
                            host, host_ranges, host_route = ia.parse_container_view_by_index(container, index, (rect, m, 0), parse_all)
                            got, ranges, route = ctx.parse_container_view_device(container, index, (rect, m, 0), parse_all)
                            what = (len(container), version, interval, m, rect, parse_all)
                            assert (route, host_route) == (0, 0), what
                            assert np.array_equal(ranges, host_ranges), what
                            assert got.shape == host.shape and np.array_equal(got, host), what
    host, _, host_route = ia.parse_container_view_by_index(blob, b"not an index", (WHOLE, 2, 0))
    got, _, route = ctx.parse_container_view_device(blob, b"not an index", (WHOLE, 2, 0))
    assert (route, host_route) == (1, 1) and np.array_equal(got, host)


def test_arguments_are_checked_before_anything_runs(ia, ctx, inputs):
    import torch
    blob, indexes, _ = inputs["main"]
    w, h = region_cases.W, region_cases.H
    good = (WHOLE, 1, 3)
    for bad, text in ((((0, 0, 8, 8), -1, 0), "frame 1: steps"), (((0, 0, 8, 8), 0, 4), "frame 1: scale_log2"), (((0, 0, 8, 8), 0, -1), "frame 1: scale_log2"),
                      (((4, 0, 8, 8), 0, 3), "frame 1: the rectangle's origin"), (((w - 3, 0, 4, 1), 0, 0), "frame 1: rectangle"),
                      (((0, 0, w, h + 1), 1, 0), "frame 1: rectangle"), (((0, 0, 0, 5), 0, 0), "frame 1: rectangle")):
        for call in (ctx.decode_views, ctx.decode_views_device):
            for index in (indexes[1], None):
                with pytest.raises(ia.MpcError) as e:
                    call([blob, blob], [index, index], [good, bad])
                assert e.value.status == ia.api.MPC_ERR_ARGUMENT and text in str(e.value), (bad, str(e.value))
    # a capacity below 3 * ceil(w / c) * ceil(h / c); bytes behind the view are left alone
    view = ((224, 64, 19, 21), 2, 2)
    need = 3 * 5 * 6
    buf = torch.full((2 * need + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    for index in (indexes[2], None):
        frames, routes = ctx.decode_views_device([blob], [index], [view], out=[buf[:need]])
        assert routes == [0 if index else 1] and tuple(frames[0].shape) == (6, 5, 3)
        assert np.array_equal(_host(frames)[0], expected_view(blob, view)) and bool((buf[need:] == 0xA5).all())
        with pytest.raises(ia.MpcError) as e:
            ctx.decode_views_device([blob, blob], [index, index], [view, view], out=[buf[:need], buf[need:2 * need - 1]])
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "frame 1: capacity" in str(e.value)
    frames, routes = ctx.decode_views([blob], [indexes[1]], [good])
    assert routes == [0] and np.array_equal(frames[0], expected_view(blob, good))
