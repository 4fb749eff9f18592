"""The tile decoder on records that no pursuit emits (run with -m gpu): the hand-made frames of record_cases.py -- forward references,
zero coefficients that unlock a block, repeated base atoms, the edges of the dynamic dictionary, extreme coefficients and steps,
exact halves in front of the rounding, sums that cancel only in double -- through every route that ends in reconstruct_tile_pixel:
the records straight into mp_decode_kernel, containers through the sequence, indexed and scan decoders, rectangles
(mp_decode_window_kernel), views (mp_decode_view_kernel) and the distortion kernel, in both flavours.  Every expected pixel is the
ORACLE's decode of the container (decode_image for the double flavour, decode_image_fast for the float one), cropped and reduced in
numpy where the route does that; every equality is exact.  test_record_cases.py shows on the CPU that these frames tell a right
decoder from ten wrong ones.

What mpc_decode_tiles_device and mpc_distortion_device do with a record outside its dictionary is not asserted: include/mpcodec.h
does not say."""
import ctypes as C

import numpy as np
import pytest

import record_cases as rc
import region_cases
import view_cases
from region_cases import crop
from view_cases import WHOLE

pytestmark = pytest.mark.gpu

NAMES = tuple(rc.FRAMES)
FLAVOURS = (False, True)
ORDER = ("wide", "odd_k", "wide_closed", "small")                   # NAMES shuffled (seed 4: a fixed order, written out)
VIEW_STEPS = (0, 1, 2, 3, 31, 32, 40)
RAGGED_COLUMN, RAGGED_ROW = (256, 0, 5, 277), (0, 272, 261, 5)


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


_contexts = {}


def _context(ia, K, fast):
    if (K, fast) not in _contexts:
        _contexts[K, fast] = ia.create_compression_context(K, 8, 3.5, device=0).set_fast(fast)
    return _contexts[K, fast]


@pytest.fixture(scope="module")
def ctx(ia):
    """by flavour: a context of K = 8 decodes a container of any K"""
    return {fast: _context(ia, 8, fast) for fast in FLAVOURS}


_wanted = {}


def _want(oracle, f, fast):
    """the oracle's decode of a frame's container, computed once"""
    if (f.name, fast) not in _wanted:
        _wanted[f.name, fast] = (oracle.decode_image_fast if fast else oracle.decode_image)(f.container)
    return _wanted[f.name, fast]


def _host(frames):
    return [np.asarray(x.cpu()) if hasattr(x, "cpu") else np.asarray(x) for x in frames]


def _indexes(ia, blob):
    return {1: ia.container_index(blob, 32), 2: ia.container_index(blob, 32, expanded=True)}


def _upload(f):
    import torch
    d_counts = torch.from_numpy(f.counts.view(np.int16).copy()).cuda()
    d_choices = torch.from_numpy(f.choices.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return d_counts, d_choices


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("name", NAMES)
def test_records_straight_into_the_kernel(ia, oracle, name, fast):
    import torch
    f = rc.frame(name)
    c = _context(ia, f.K, fast)
    d_counts, d_choices = _upload(f)
    out = torch.zeros((f.H, f.W, 3), dtype=torch.uint8, device="cuda")
    q = np.ascontiguousarray(f.quant, np.float64)                   # the header's u16 tables
    st = c.L.mpc_decode_tiles_device(c.h, d_counts.data_ptr(), d_choices.data_ptr(), q.ctypes.data_as(C.POINTER(C.c_double)), f.W, f.H,
                                     out.data_ptr(), None)
    assert st == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _want(oracle, f, fast))


@pytest.mark.parametrize("fast", FLAVOURS)
def test_container_routes(ia, oracle, ctx, fast):
    c = ctx[fast]
    frames = [rc.frame(name) for name in ORDER]
    assert sorted(ORDER) == sorted(NAMES)
    blobs = [f.container for f in frames]
    want = [_want(oracle, f, fast) for f in frames]
    assert (want[0] != _want(oracle, frames[0], not fast)).any()    # the two flavours are told apart
    got = {"decode_image": [np.asarray(ia.decode_image(b, c)) for b in blobs],
           "decode_images": _host(c.decode_images(blobs)),
           "decode_images_device": _host(c.decode_images_device(blobs))}
    for version in (1, 2):
        indexes = [_indexes(ia, b)[version] for b in blobs]
        for call in (c.decode_images_indexed, c.decode_images_indexed_device):
            out, routes = call(blobs, indexes)
            assert routes == [0] * len(blobs), (call.__name__, version, routes)
            got[call.__name__, version] = _host(out)
    out, routes = c.decode_images_scan(blobs)
    assert set(routes) <= {0, 1}
    got["decode_images_scan"] = _host(out)
    for route, pixels in got.items():
        for f, mine, exp in zip(frames, pixels, want):
            assert mine.shape == exp.shape and np.array_equal(mine, exp), (route, f.name)


def _forward_tile(f):
    """a tile whose luma list names a row before the base choice that unlocks it"""
    return next(t for t in range(len(f.records)) if any(rc.outside(f.records[t][0][:n]) for n in range(1, len(f.records[t][0]))))


@pytest.mark.parametrize("fast", FLAVOURS)
def test_regions(ia, oracle, ctx, fast):
    c = ctx[fast]
    f = rc.frame("wide")
    x, y, w, h = f.tile_of(_forward_tile(f))
    assert (w, h) == (8, 8)
    rects = [region_cases.ACROSS_1024, RAGGED_COLUMN, RAGGED_ROW, (100, 200, 1, 1), (x + 2, y + 3, 5, 4), (0, 0, f.W, f.H)]
    n = len(rects)
    full = _want(oracle, f, fast)
    index = _indexes(ia, f.container)[2]
    for parse_all in (False, True):
        for call in (c.decode_regions, c.decode_regions_device):
            out, routes = call([f.container] * n, [index] * n, rects, parse_all)
            assert routes == [0] * n, (call.__name__, parse_all, routes)
            for mine, rect in zip(_host(out), rects):
                assert np.array_equal(mine, crop(full, rect)), (call.__name__, parse_all, rect)


@pytest.mark.parametrize("fast", FLAVOURS)
def test_views_of_the_closed_frame(ia, oracle, ctx, fast):
    c = ctx[fast]
    f = rc.frame("wide_closed")
    blob = f.container
    views = [(rect, m, s) for rect in (WHOLE, region_cases.ACROSS_1024) for m in VIEW_STEPS for s in view_cases.SCALES]
    n = len(views)
    want = [view_cases.expected_view(blob, view, fast) for view in views]
    index = _indexes(ia, blob)[2]
    for call in (c.decode_views, c.decode_views_device):
        out, routes = call([blob] * n, [index] * n, views)
        assert routes == [0] * n, (call.__name__, routes)
        for mine, exp, view in zip(_host(out), want, views):
            assert mine.shape == exp.shape and np.array_equal(mine, exp), (call.__name__, view)


@pytest.mark.parametrize("fast", FLAVOURS)
def test_views_of_the_frame_with_forward_references(ia, oracle, ctx, fast):
    c = ctx[fast]
    f = rc.frame("wide")
    blob = f.container
    full = _want(oracle, f, fast)
    index = _indexes(ia, blob)[2]
    views = [(WHOLE, 0, s) for s in view_cases.SCALES]
    for call in (c.decode_views, c.decode_views_device):
        out, routes = call([blob] * 4, [index] * 4, views)
        assert routes == [0] * 4
        for mine, (_, _, s) in zip(_host(out), views):
            assert np.array_equal(mine, view_cases.reduce(full, s)), (call.__name__, s)
    # one step: the first record of a Forward list names a row of a block that only a later base choice unlocks
    assert any(rc.outside(lst[:1]) for per_channel in f.records for lst in per_channel)
    for call in (c.decode_views, c.decode_views_device):
        for parse_all in (False, True):
            for with_index in (index, None):
                with pytest.raises(ia.MpcError) as e:
                    call([blob], [with_index], [(WHOLE, 1, 0)], parse_all)
                assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("frame 0: Invalid bitstream"), str(e.value)
    out, _ = c.decode_views([blob], [index], [(WHOLE, 0, 0)])       # and the context is as good as before
    assert np.array_equal(_host(out)[0], full)


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("name", ("small", "wide"))
def test_distortion(ia, oracle, name, fast):
    import torch
    f = rc.frame(name)
    c = _context(ia, f.K, fast)
    rgb = np.random.default_rng(rc.SEED).integers(0, 256, (f.H, f.W, 3)).astype(np.uint8)
    d_counts, d_choices = _upload(f)
    d_rgb = torch.from_numpy(rgb).cuda()
    tiles = f.tiles_x * f.tiles_y
    d_sse = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_tiles = torch.zeros(tiles, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.distortion_device(d_counts.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), f.W, f.H, d_sse.data_ptr(), d_tiles.data_ptr(),
                        quant=f.quant.astype(np.float64))
    torch.cuda.synchronize()
    d = (rgb.astype(np.int64) - _want(oracle, f, fast).astype(np.int64)) ** 2
    want = np.array([d[f.tile_mask([t])].sum() for t in range(tiles)], np.int64)
    assert np.array_equal(d_tiles.cpu().numpy().view(np.uint32).astype(np.int64), want)
    assert int(d_sse.item()) == int(want.sum()) == int(d.sum())


def _other_tile(b):
    """the rectangle of a tile in another tile column and another tile row than the bad one"""
    tx, ty = divmod(b.bad_at[0], b.tiles_y)
    return b.tile_of(((tx + 2) % b.tiles_x) * b.tiles_y + (ty + 1) % b.tiles_y)


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("kind,ch,last", rc.bad_cases())
def test_refusals(ia, oracle, ctx, kind, ch, last, fast):
    c = ctx[fast]
    good = rc.frame("small")
    b = rc.bad("small", kind, ch, last)
    want = _want(oracle, good, fast)
    with pytest.raises(ia.MpcError) as e:
        ia.decode_image(b.container, c)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM
    with pytest.raises(ia.MpcError) as e:
        c.decode_images([good.container, b.container, good.container])
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and "frame 1: " in str(e.value), str(e.value)
    assert np.array_equal(np.asarray(ia.decode_image(good.container, c)), want)
    # a rectangle that does not touch the bad tile: the oracle skips the bad step, and nothing outside that tile depends on it
    index = _indexes(ia, b.container)[2]
    away, at = _other_tile(b), b.tile_of(b.bad_at[0])
    skipped = _want(oracle, b, fast)
    assert np.array_equal(crop(skipped, away), crop(want, away))
    for call in (c.decode_regions, c.decode_regions_device):
        out, routes = call([b.container], [index], [away])
        assert routes == [0] and np.array_equal(_host(out)[0], crop(skipped, away)), call.__name__
        for rect in (at, (0, 0, b.W, b.H)):
            with pytest.raises(ia.MpcError) as e:
                call([b.container], [index], [rect])
            assert e.value.status == ia.api.MPC_ERR_BITSTREAM, (call.__name__, rect)
    if kind != "beyond":
        return
    # the same record one row lower is the last row of its dictionary: every route decodes it
    twin = rc.bad("small", kind, ch, last, lower=1)
    blob, exp = twin.container, _want(oracle, twin, fast)
    indexes = _indexes(ia, blob)
    got = [np.asarray(ia.decode_image(blob, c)), _host(c.decode_images([blob]))[0], _host(c.decode_images_device([blob]))[0],
           _host(c.decode_images_scan([blob])[0])[0]]
    for version in (1, 2):
        got += [_host(c.decode_images_indexed([blob], [indexes[version]])[0])[0], _host(c.decode_images_indexed_device([blob], [indexes[version]])[0])[0]]
    for call in (c.decode_regions, c.decode_regions_device):
        got.append(_host(call([blob], [indexes[2]], [(0, 0, twin.W, twin.H)])[0])[0])
        assert np.array_equal(_host(call([blob], [indexes[2]], [at])[0])[0], crop(exp, at))
    for call in (c.decode_views, c.decode_views_device):
        got.append(_host(call([blob], [indexes[2]], [(WHOLE, 0, 0)])[0])[0])
    for n, mine in enumerate(got):
        assert np.array_equal(mine, exp), n
