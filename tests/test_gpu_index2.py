"""Region decodes through index version 2 on the GPU (run with -m gpu): run-length packed and step-0 coefficient streams cut by
their aux entries.  Both entry points and both flags against the crop of the whole frame's decode, the device's windowed parse
and its chunk table against their definitions on the host, chunks that are never read, damaged aux sections.  Every equality is
exact."""
import numpy as np
import pytest

import index2_cases as cases
import region_cases
from region_cases import ACROSS_1024, crop

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
    c = ia.create_compression_context(region_cases.K, 8, region_cases.QUALITY, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def f1(ia, ctx):
    """{interval: (container, version 1, version 2)} of F1 from the indexed encoder and index_extend, and the whole decode"""
    out = {}
    for interval in cases.F1_INTERVALS:
        blob, v1 = ctx.encode_images_indexed([region_cases.frame()], interval)[0]
        v2 = ia.index_extend(blob, v1)
        assert v2 == ia.container_index(blob, interval, expanded=True) and ia.index_version(v2) == 2
        out[interval] = (blob, v1, v2)
    return out, _host(ctx.decode_images([out[32][0]]))[0]


@pytest.fixture(scope="module")
def f2(ia):
    ctx32 = ia.create_compression_context(cases.F2_K, 8, cases.F2_QUALITY, device=0)
    blob, v1 = ctx32.encode_images_indexed([cases.f2_frame()], cases.F2_INTERVAL)[0]
    v2 = ia.index_extend(blob, v1)
    assert v2 == ia.container_index(blob, cases.F2_INTERVAL, expanded=True)
    yield ctx32, blob, v1, v2, _host(ctx32.decode_images([blob]))[0]
    ctx32.close()


def _host(frames):
    return [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in frames]


def _check_regions(ctx, blobs, indexes, rects, fulls, flags=(False, True)):
    """both entry points, both flags: the exact crops, route 0"""
    want = [crop(full, rect) for full, rect in zip(fulls, rects)]
    for parse_all in flags:
        for call in (ctx.decode_regions, ctx.decode_regions_device):
            frames, routes = call(blobs, indexes, rects, parse_all)
            assert routes == [0] * len(rects), (call.__name__, parse_all, routes)
            for n, (got, exp) in enumerate(zip(_host(frames), want)):
                assert got.shape == exp.shape and np.array_equal(got, exp), (call.__name__, parse_all, n, rects[n])


def test_the_frames_cover_what_they_are_meant_to(ia, f1, f2):
    """the containers the device encoder wrote have the streams these tests are about (index2_cases.check_coverage, run by the
    host tests, says the same of the oracle's containers)"""
    assert len(cases.inside(f1[0][32][0], 32, ACROSS_1024)) >= 20
    assert {g[3] for g in cases.inside(f1[0][32][0], 32, ACROSS_1024)} == {0, 1, 2}
    got = cases.inside(f2[1], cases.F2_INTERVAL, cases.F2_INNER)
    assert len([g for g in got if g[1] * cases.F2_INTERVAL > 2048 and (g[1] * cases.F2_INTERVAL) % 2048]) >= 4


@pytest.mark.parametrize("interval", cases.F1_INTERVALS)
def test_every_rectangle_of_f1(ia, ctx, f1, interval):
    blob, _, v2 = f1[0][interval]
    rects = list(region_cases.RECTS)
    n = len(rects)
    _check_regions(ctx, [blob] * n, [v2] * n, rects, [f1[1]] * n)
    for rect in rects:                                              # one frame a call as well: the calling thread's own path
        _check_regions(ctx, [blob], [v2], [rect], [f1[1]], flags=(False,))


def test_rectangles_of_f2(ia, f2):
    ctx32, blob, _, v2, full = f2
    rects = list(cases.F2_RECTS)
    _check_regions(ctx32, [blob] * 3, [v2] * 3, rects, [full] * 3)
    for rect in rects:
        _check_regions(ctx32, [blob], [v2], [rect], [full], flags=(False,))


def test_float_flavour(ia, oracle, f1):
    blob, _, v2 = f1[0][32]
    fast = ia.create_compression_context(region_cases.K, 8, region_cases.QUALITY, device=0).set_fast(True)
    full = oracle.decode_image_fast(blob)
    rects = list(region_cases.RECTS)
    n = len(rects)
    _check_regions(fast, [blob] * n, [v2] * n, rects, [full] * n, flags=(False,))
    fast.close()


def _check_device_half(ia, ctx, blob, v2, rects, flags=(False, True)):
    for rect in rects:
        for parse_all in flags:
            host, host_ranges, host_route = ia.parse_container_window_by_index(blob, v2, rect, parse_all)
            got, ranges, route = ctx.parse_container_window_device(blob, v2, rect, parse_all)
            what = (rect, parse_all)
            assert (route, host_route) == (0, 0), what
            assert np.array_equal(ranges, host_ranges), what
            assert got.shape == host.shape and np.array_equal(got, host), what
            chunks, chunks_route = ctx.window_chunks_device(blob, v2, rect, parse_all)
            host_chunks, host_chunks_route = ia.window_chunks_by_index(blob, v2, rect, parse_all)
            assert (chunks_route, host_chunks_route) == (0, 0) and np.array_equal(chunks, host_chunks), what


@pytest.mark.parametrize("interval", cases.F1_INTERVALS)
def test_device_half_is_the_hosts_f1(ia, ctx, f1, interval):
    blob, v1, v2 = f1[0][interval]
    _check_device_half(ia, ctx, blob, v2, region_cases.RECTS)
    chunks, route = ctx.window_chunks_device(blob, v1, ACROSS_1024)                             # a version-1 index: as before
    assert route == 0 and np.array_equal(chunks, cases.expected_chunks(blob, interval, ACROSS_1024, 1))


def test_device_half_is_the_hosts_f2(ia, f2):
    ctx32, blob, _, v2, _ = f2
    _check_device_half(ia, ctx32, blob, v2, cases.F2_RECTS, flags=(False,))
    assert np.array_equal(ctx32.window_chunks_device(blob, v2, cases.F2_INNER)[0], cases.expected_chunks(blob, cases.F2_INTERVAL, cases.F2_INNER, 2))


def test_chunks_outside_the_range_are_never_read(ia, ctx, f1):
    blob, v1, v2 = f1[0][32]
    want = crop(f1[1], ACROSS_1024)
    damaged = cases.never_read_containers(ia, v1)
    n = len(damaged)
    for call in (ctx.decode_regions, ctx.decode_regions_device):
        frames, routes = call([x for _, x in damaged], [v2] * n, [ACROSS_1024] * n)
        assert routes == [0] * n
        for (what, _), got in zip(damaged, _host(frames)):
            assert np.array_equal(got, want), what


def test_damaged_aux(ia, ctx, oracle, f1):
    """the device refuses what the host's definition refuses, gives its symbols where it does not, and decodes afterwards"""
    blob, v1, v2 = f1[0][32]
    rect = ACROSS_1024
    damaged = cases.damaged_v2(ia, oracle, v1, v2) + cases.exit_flips(ia, blob, v2, v1, 32, rect)
    want = crop(f1[1], rect)
    refused = 0
    for k in range(0, len(damaged), 8):
        some = damaged[k:k + 8]
        hosts = [ia.parse_container_window_by_index(blob, bad, rect) for _, bad in some]
        call = ctx.decode_regions if (k // 8) % 2 == 0 else ctx.decode_regions_device
        frames, routes = call([blob] * len(some), [bad for _, bad in some], [rect] * len(some))
        assert routes == [h[2] for h in hosts], [w for w, _ in some]
        for (what, bad), got, route in zip(some, _host(frames), routes):
            if route == 1:
                refused += 1
                assert np.array_equal(got, want), what
        frames, routes = call([blob] * len(some), [bad for _, bad in some], [rect] * len(some), True)
        for (what, _), got in zip(some, _host(frames)):
            assert np.array_equal(got, want), what
    assert refused >= 20, refused
    for what, bad in damaged[::5]:
        host, _, host_route = ia.parse_container_window_by_index(blob, bad, rect)
        got, _, route = ctx.parse_container_window_device(blob, bad, rect)
        assert route == host_route and np.array_equal(got, host), what
    _check_regions(ctx, [blob], [v2], [rect], [f1[1]])


def test_guard_band(ia, ctx, f1):
    import torch
    blob, _, v2 = f1[0][32]
    for rect in (ACROSS_1024, (5, 3, 50, 70), (120, 50, 20, 20)):
        need = 3 * rect[2] * rect[3]
        buf = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
        frames, routes = ctx.decode_regions_device([blob], [v2], [rect], out=[buf[:need]])
        assert routes == [0]
        assert np.array_equal(_host(frames)[0], crop(f1[1], rect))
        assert bool((buf[need:] == 0xA5).all()), rect


def test_whole_frame_decodes_take_version_2_as_version_1(ia, ctx, oracle, f1):
    blob, v1, v2 = f1[0][32]
    # aux entries that keep their structure (a bit of `prev` of a packed stream's entry c0) and random flips of the section
    kept = [cases.flip(v2, 8 * cases.aux_entry_offset(ia, v2, v1, i + 1, c0) + 64 + 1) for i, c0, _, _ in cases.inside(blob, 32, ACROSS_1024)[:3]]
    assert [ia.index_version(bad) for bad in kept] == [2, 2, 2]
    damaged = kept + [bad for _, bad in cases.damaged_aux(ia, v2, v1, 1, count=3)]
    indexes = [v2, v1] + damaged
    n = len(indexes)
    want_routes = [0, 0] + [0 if ia.index_version(bad) == 2 else 1 for bad in damaged]
    assert 0 in want_routes[2:]
    for call in (ctx.decode_images_indexed, ctx.decode_images_indexed_device):
        frames, routes = call([blob] * n, indexes)
        assert list(routes) == want_routes, call.__name__
        for got in _host(frames):
            assert np.array_equal(got, f1[1]), call.__name__
    for index in indexes[:4]:
        a, route_a = ctx.parse_container_device(blob, index)
        b, route_b = ctx.parse_container_device(blob, v1)
        assert np.array_equal(a, b) and route_b == 0 and route_a == (0 if ia.index_version(index) else 1)
