"""Compose on the GPU (run with -m gpu): mpc_compose_indexed against its definition on the host (compose_container) through both
routes, both flags and both index versions; pixel parts against the device encoder's container of the pasted pixels; the seek index
that comes with the result; the paste kernel on hand-made records against numpy; damaged indexes and containers; refusals; and the
context afterwards.  Every equality is exact.

The shapes are the smallest that can still go wrong: 261x277 at K = 8 is 33 x 35 = 1 155 tiles, ragged both ways, across gather block
1024 (compose_cases.check_coverage); 1003x517 at K = 32 is eight gather blocks."""
import numpy as np
import pytest

import compose_cases as cc
import parse_cases
import region_cases
from container_cases import FRAMES, corpus as _corpus

pytestmark = pytest.mark.gpu

KEYS = [(version, interval) for version in (1, 2) for interval in region_cases.INTERVALS] + [(0, 0), (-1, 0)]


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def ctx(ia):
    return ia.create_compression_context(cc.K, 8, cc.QUALITY, device=0)


@pytest.fixture(scope="module")
def definition(ia, oracle):
    """{name: compose_container's bytes}: computed once, shared, never changed"""
    cc.check_coverage(ia)
    return {name: ia.compose_container(*cc.lists()[name]) for name in cc.NAMES}


_INDEXES = {}


def _index(ia, blob, key):
    """the seek index of a blob: key = (version, interval), version 0 = none, -1 = garbage"""
    version, interval = key
    if version == 0:
        return None
    if version < 0:
        return b"not an index at all, whatever its length may be"
    if (blob, key) not in _INDEXES:
        _INDEXES[blob, key] = ia.container_index(blob, interval, expanded=version == 2)
    return _INDEXES[blob, key]


def _routes(blobs, parts, width, height, route):
    owner = cc.owners(blobs, parts, width, height)
    return [route if (owner == p).any() else -1 for p in range(len(parts))]


def test_device_is_the_definition(ia, ctx, definition):
    for name in cc.NAMES:
        blobs, parts, width, height = cc.lists()[name]
        for key in KEYS:
            want_routes = _routes(blobs, parts, width, height, 0 if key[0] > 0 else 1)
            idx = [_index(ia, b, key) for b in blobs]
            for parse_all in (False, True):
                got, index, routes = ctx.compose(blobs, idx, parts, width, height, parse_all)
                assert routes == want_routes, (name, key, parse_all, routes)
                assert index is None and got == definition[name], (name, key, parse_all)
    # the index array may be missing altogether, or only some of its entries
    blobs, parts, width, height = cc.lists()["overlap"]
    assert ctx.compose(blobs, None, parts, width, height) == (definition["overlap"], None, [-1, 1, 1, 1])
    got, _, routes = ctx.compose(blobs, [None, _index(ia, blobs[1], (2, 32))], parts, width, height)
    assert got == definition["overlap"] and routes == [-1, 1, 0, 1]


def _edit_parts(rect, pixels):
    return [(0, None, 0, 0), (pixels, None, rect[0], rect[1])]


def test_pixel_parts(ia, ctx, oracle):
    import torch
    main, frame, other = cc.container(), cc.frame(), cc.other_frame()
    assert ctx.encode_images([frame]) == [main]
    d_other = torch.from_numpy(other).cuda()
    for n, rect in enumerate(cc.EDITS):
        x, y, w, h = rect
        want = ctx.encode_images([cc.edited(rect)])[0]
        assert want != main
        view = other[y:y + h, x:x + w]                              # a strided view of the larger array
        assert view.strides[0] == 3 * cc.W
        key = KEYS[n % len(KEYS)]
        route = 0 if key[0] > 0 else 1
        for pixels in (np.ascontiguousarray(view), view):
            got, _, routes = ctx.compose([main], [_index(ia, main, key)], _edit_parts(rect, pixels), cc.W, cc.H)
            assert got == want and routes == [route, 2], (rect, key)
        on_device = (d_other.data_ptr() + 3 * (y * cc.W + x), w, h, 3 * cc.W)
        got, _, routes = ctx.compose([main], [_index(ia, main, key)], _edit_parts(rect, on_device), cc.W, cc.H, device_pixels=True)
        assert got == want and routes == [route, 2], (rect, key)
    # no container at all: an encode from patches, with the context's tables
    cx, cy = cc.CUT_X, cc.CUT_Y
    mosaic = [(frame[:cy, :cx], None, 0, 0), (frame[:cy, cx:], None, cx, 0), (frame[cy:, :cx], None, 0, cy), (frame[cy:, cx:], None, cx, cy)]
    assert ctx.compose([], [], mosaic, cc.W, cc.H) == (main, None, [2, 2, 2, 2])
    # a pixel part and a container part that overlap, in both orders: the later one wins the tiles they share
    other_blob = cc.other_container()
    band = np.ascontiguousarray(other[:, 96:176])
    rect = (40, 64, 168, 96)
    for order in (0, 1):
        over = [(1, rect, 40, 64), (band, None, 96, 0)][::1 if order == 0 else -1]
        parts = [(0, None, 0, 0)] + over
        want = ctx.encode_images([cc.pasted((frame, other), parts, cc.W, cc.H)])[0]
        got, _, routes = ctx.compose([main, other_blob], [_index(ia, main, (2, 32)), None], parts, cc.W, cc.H)
        assert got == want and routes == [0] + [1, 2][::1 if order == 0 else -1], order
    # a pixel part that owns no tile is skipped
    got, _, routes = ctx.compose([main], None, [(band, None, 96, 0), (0, None, 0, 0)], cc.W, cc.H)
    assert got == main and routes == [-1, 1]


def test_a_fast_context(ia, definition):
    fast = ia.create_compression_context(cc.K, 8, cc.QUALITY, device=0).set_fast(True)
    for name in cc.NAMES:
        blobs, parts, width, height = cc.lists()[name]
        for key in ((2, 32), (0, 0)):
            got, _, _ = fast.compose(blobs, [_index(ia, b, key) for b in blobs], parts, width, height)
            assert got == definition[name], (name, key)
    rect = cc.EDITS[1]
    x, y, w, h = rect
    base = fast.encode_images([cc.frame()])[0]                      # the float pursuit's container of the frame
    want = fast.encode_images([cc.edited(rect)])[0]
    got, _, routes = fast.compose([base], None, _edit_parts(rect, cc.other_frame()[y:y + h, x:x + w]), cc.W, cc.H)
    assert got == want and routes == [1, 2]
    fast.close()


def test_the_index_comes_with_the_result(ia, ctx, definition):
    name = "edit %s" % (cc.EDITS[1],)
    blobs, parts, width, height = cc.lists()[name]
    idx = [_index(ia, b, (2, 32)) for b in blobs]
    pixels = np.asarray(ctx.decode_images([definition[name]])[0])
    for interval in (32, 100, 0):
        got, index, _ = ctx.compose(blobs, idx, parts, width, height, index_interval=interval)
        assert got == definition[name]
        assert index == ia.container_index(got, interval, expanded=True), interval
        rects = list(region_cases.RECTS[3:6])
        regions, routes = ctx.decode_regions([got] * len(rects), [index] * len(rects), rects)
        assert routes == [0] * len(rects)
        for rect, region in zip(rects, regions):
            assert np.array_equal(np.asarray(region), region_cases.crop(pixels, rect)), (interval, rect)
    with pytest.raises(ia.MpcError) as e:
        ctx.compose(blobs, idx, parts, width, height, index_interval=3)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "interval" in str(e.value)


def test_eight_gather_blocks(ia, oracle):
    w, h, k, _ = FRAMES[3]
    assert (w, h, k) == (1003, 517, 32) and -(-(-(-w // 8) * -(-h // 8)) // 1024) == 8
    big = ia.create_compression_context(k, 8, 3.5, device=0)
    frame, other = oracle.synth_frame(w, h, 103).copy(), oracle.synth_frame(w, h, 104).copy()
    blob, other_blob = big.encode_images([frame, other])
    # one edit across a block boundary: columns 14 - 16 of 65 rows hold tile 1024
    rect = (112, 200, 24, 80)
    t0, t1, _ = region_cases.tile_range(rect, h)
    assert t0 < 1024 < t1
    x, y, rw, rh = rect
    edited = frame.copy()
    edited[y:y + rh, x:x + rw] = other[y:y + rh, x:x + rw]
    want = big.encode_images([edited])[0]
    parts = [(0, None, 0, 0), (1, rect, x, y)]
    assert ia.compose_container([blob, other_blob], parts, w, h) == want
    for key in ((2, 0), (1, 32), (0, 0)):
        for parse_all in (False, True):
            got, _, routes = big.compose([blob, other_blob], [_index(ia, b, key) for b in (blob, other_blob)], parts, w, h, parse_all)
            assert got == want and routes == [0 if key[0] > 0 else 1] * 2, (key, parse_all)
    got, _, routes = big.compose([blob], None, [(0, None, 0, 0), (other[y:y + rh, x:x + rw], None, x, y)], w, h)
    assert got == want and routes == [1, 2]
    # the quadrant identity
    cx, cy = 504, 256
    rects = ((0, 0, cx, cy), (cx, 0, w - cx, cy), (0, cy, cx, h - cy), (cx, cy, w - cx, h - cy))
    quads = [ia.transcode_container(blob, (r, 0, 0)) for r in rects]
    parts = [(i, None, r[0], r[1]) for i, r in enumerate(rects)]
    for key in ((2, 0), (0, 0)):
        got, _, routes = big.compose(quads, [_index(ia, b, key) for b in quads], parts, w, h)
        assert got == blob and routes == [0 if key[0] > 0 else 1] * 4, key
    big.close()


def _paste_numpy(counts, choices, src_ty, src_grid, dst_counts, dst_choices, dst_ty, dst_at, k, owner, part):
    """the paste on numpy records: [tiles, 3] and [tiles, 3, K] on either side, changed in place"""
    tx0, tx1, ty0, ty1 = src_grid
    src = (np.arange(tx0, tx1)[:, None] * src_ty + np.arange(ty0, ty1)[None, :]).reshape(-1)
    dst = ((np.arange(tx0, tx1) - tx0 + dst_at[0])[:, None] * dst_ty + (np.arange(ty0, ty1) - ty0 + dst_at[1])[None, :]).reshape(-1)
    if owner is not None:
        keep = owner[dst] == part
        src, dst = src[keep], dst[keep]
    c = np.minimum(counts[src].astype(np.int64), k)
    dst_counts[dst] = c.astype(np.uint16)
    dst_choices[dst] = np.where(np.arange(k)[None, None, :] < c[:, :, None], choices[src], 0).astype(np.uint32)


@pytest.mark.parametrize("k,w,h", ((3, 24, 40), (8, 261, 277)))
def test_paste_records_on_hand_made_records(ia, k, w, h):
    """random records with counts 0 ... K and garbage behind every count, into a destination of another tile height that is filled with
    a pattern: the kernel writes the tiles of the grid it owns, whole, and nothing else"""
    import torch
    paste = ia.create_compression_context(k, 8, 3.5, device=0)
    dw, dh = w + 16, h + 24                                         # ragged where the source is; 3 more tile rows
    tx, ty, dtx, dty = -(-w // 8), -(-h // 8), -(-dw // 8), -(-dh // 8)
    assert dty != ty
    tiles, dtiles = tx * ty, dtx * dty
    rng = np.random.default_rng([20261019, k])
    counts = rng.integers(0, k + 1, (tiles, 3)).astype(np.uint16)
    choices = rng.integers(1, 2**32, (tiles, 3, k), dtype=np.uint64).astype(np.uint32)
    owner = rng.integers(0, 3, dtiles).astype(np.int32)             # part 1 owns about a third of the destination
    d_counts = torch.from_numpy(counts.view(np.int16)).cuda()
    d_choices = torch.from_numpy(choices.view(np.int32)).cuda()
    guard = 64                                                      # words in front of and behind the destination, which must stay as they are

    def run(rect, at, owned, dc=d_counts, expect_status=None):
        out_counts = torch.full((2 * guard + 3 * dtiles,), 0x5A5A, dtype=torch.int16, device="cuda")
        out_choices = torch.full((2 * guard + 3 * dtiles * k,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        error = None
        try:
            paste.paste_records_device(dc.data_ptr(), d_choices.data_ptr(), w, h, rect, out_counts[guard:].data_ptr(),
                                       out_choices[guard:].data_ptr(), dw, dh, at[0], at[1], d_owner.data_ptr() if owned else None, 1)
        except ia.MpcError as e:
            error = e
        torch.cuda.synchronize()
        oc, ox = out_counts.cpu().numpy().view(np.uint16), out_choices.cpu().numpy().view(np.uint32)
        assert (oc[:guard] == 0x5A5A).all() and (oc[guard + 3 * dtiles:] == 0x5A5A).all(), (rect, at)
        assert (ox[:guard] == 0x5A5A5A5A).all() and (ox[guard + 3 * dtiles * k:] == 0x5A5A5A5A).all(), (rect, at)
        return oc[guard:guard + 3 * dtiles].reshape(dtiles, 3), ox[guard:guard + 3 * dtiles * k].reshape(dtiles, 3, k), error

    def want(rect, at, owned, src_counts=counts):
        x, y, rw, rh = rect if rect else (0, 0, w, h)
        grid = (x // 8, -(-(x + rw) // 8), y // 8, -(-(y + rh) // 8))
        wc = np.full((dtiles, 3), 0x5A5A, np.uint16)
        wx = np.full((dtiles, 3, k), 0x5A5A5A5A, np.uint32)
        _paste_numpy(src_counts, choices, ty, grid, wc, wx, dty, (at[0] // 8, at[1] // 8), k, owner if owned else None, 1)
        return wc, wx

    corner = (8 * (tx - 2), 8 * (ty - 2), w - 8 * (tx - 2), h - 8 * (ty - 2))          # two by two tiles, ragged where the frame is
    x0 = 8 * max(tx - 5, 0)
    across = (x0, 8, w - x0, 8 * (ty - 2))                                              # the last columns but for a row at each end
    cases = ((None, (16, 24)), ((0, 0, w, h), (16, 24)),                                # the whole source: its ragged edges on the destination's
             ((8, 16, 8, 8), (16, 8)), ((8, 16, 8, 8), (0, 0)),                         # one tile
             (corner, (dw - corner[2], dh - corner[3])),                                # the ragged corner to the ragged corner
             (across, (x0 + 16, 16)), ((0, 0, 16, 8 * (ty - 1)), (8, 24)))
    for rect, at in cases:                                          # every grid has a tile that part 1 owns; the larger ones one it does not
        x, y, rw, rh = rect if rect else (0, 0, w, h)
        first = (at[0] // 8) * dty + at[1] // 8
        owner[first] = 1
        if -(-(y + rh) // 8) - y // 8 > 1:
            owner[first + 1] = 0
    d_owner = torch.from_numpy(owner).cuda()
    for rect, at in cases:
        for owned in (False, True):
            got_counts, got_choices, error = run(rect, at, owned)
            want_counts, want_choices = want(rect, at, owned)
            assert error is None, (rect, at, str(error))
            assert np.array_equal(got_counts, want_counts), (rect, at, owned)
            assert np.array_equal(got_choices, want_choices), (rect, at, owned)
            touched = (want_counts != 0x5A5A).any(axis=1)
            assert 0 < touched.sum() < dtiles                       # untouched tiles kept the pattern, and some were written
    if tiles > 1024:
        t0, t1, _ = region_cases.tile_range(across, h)
        assert t0 < 1024 < t1
    # a count of K + 1 inside the rectangle: used as K, the error word raised, then cleared by the check
    bad = counts.copy()
    bad[ty + 2, 1] = k + 1
    d_bad = torch.from_numpy(bad.view(np.int16)).cuda()
    got_counts, got_choices, error = run((8, 16, 8, 8), (16, 8), False, d_bad)
    assert error is not None and error.status == ia.api.MPC_ERR_BITSTREAM and str(error).endswith("Invalid bitstream")
    want_counts, want_choices = want((8, 16, 8, 8), (16, 8), False, np.minimum(bad, k))
    assert np.array_equal(got_counts, want_counts) and np.array_equal(got_choices, want_choices)
    # ... outside the rectangle it is never looked at
    got_counts, got_choices, error = run((0, 0, 8, 8), (0, 0), False, d_bad)
    want_counts, want_choices = want((0, 0, 8, 8), (0, 0), False)
    assert error is None and np.array_equal(got_counts, want_counts) and np.array_equal(got_choices, want_choices)
    # arguments: nothing is enqueued, the destination keeps its pattern
    refused = (((4, 0, 8, 8), (0, 0)), ((0, 0, 12, 8), (0, 0)), ((0, 0, w + 8, 8), (0, 0)), ((0, 0, 0, 8), (0, 0)), ((0, 0, 8, 8), (4, 0)),
               ((0, 0, 8, 8), (0, 3)), ((0, 0, 8, 8), (dw, 0)), ((0, 0, 16, 8), (8 * (dtx - 1), 0)), ((0, 0, 8, 8), (-8, 0)),
               ((0, 0, 8, 8), (2**31 - 8, 0)))
    if w % 8:
        refused += ((None, (0, 0)), (corner, (0, 0)))               # a ragged edge that lands inside the destination
    for rect, at in refused:
        got_counts, got_choices, error = run(rect, at, False)
        assert error is not None and error.status == ia.api.MPC_ERR_ARGUMENT, (rect, at)
        assert (got_counts == 0x5A5A).all() and (got_choices == 0x5A5A5A5A).all(), (rect, at)
    paste.close()


def test_damaged_indexes(ia, ctx, definition):
    name = "edit %s" % (cc.EDITS[0],)
    blobs, parts, width, height = cc.lists()[name]
    main, other = blobs
    stranger = ia.container_index(other, 32)
    by_route = [0, 0]
    for version in (1, 2):
        damaged = parse_cases.damaged_indexes(_index(ia, main, (version, 32)), stranger, version)
        for what, bad in damaged[::2]:
            for parse_all in (True, False):
                got, _, routes = ctx.compose(blobs, [bad, None], parts, width, height, parse_all)
                assert routes[0] in (0, 1) and routes[1] == 1, what
                if routes[0] == 1 or parse_all:
                    assert got == definition[name], (version, what, parse_all)
                by_route[routes[0]] += 1
    assert by_route[0] >= 1 and by_route[1] >= 4, by_route


def test_damaged_containers_as_overlay(ia, ctx, oracle):
    """a slice of the corpus, the containers of this context's K, over their own sound original: the definition's status and text"""
    seen = set()
    for n, blob, xs in _corpus(oracle):
        if FRAMES[n][2] != cc.K:
            continue
        w, h, _, _ = ia.container_info(blob)
        index = ia.container_index(blob, 32, expanded=True)
        parts = [(0, None, 0, 0), (1, (0, 0, 8, 8), 0, 0)]
        for k, x in list(enumerate(xs))[::4]:
            try:
                want = ia.compose_container([blob, x], parts, w, h)
            except ia.MpcError as e:
                want = e
            for idx in (None, index):
                if isinstance(want, ia.MpcError):
                    with pytest.raises(ia.MpcError) as e:
                        ctx.compose([blob, x], [index, idx], parts, w, h, parse_all=True)
                    assert e.value.status == want.status and str(e.value) == str(want), (n, k, str(e.value), str(want))
                    seen.add((want.status, cc.text_of(want)))
                else:
                    got, _, _ = ctx.compose([blob, x], [index, idx], parts, w, h, parse_all=True)
                    assert got == want, (n, k)
    assert (ia.api.MPC_ERR_BITSTREAM, "part 1: Invalid input data") in seen, seen
    # a length above K, anywhere in the source of an owning part
    bad = cc.length_above_K()
    for index in (None, ia.container_index(bad, 32, expanded=True)):
        for parse_all in (False, True):
            with pytest.raises(ia.MpcError) as e:
                ctx.compose([cc.container(), bad], [None, index], [(0, None, 0, 0), (1, (0, 0, 8, 8), 0, 0)], cc.W, cc.H, parse_all)
            assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith(": part 1: Invalid bitstream"), parse_all


def test_refusals_and_the_context_afterwards(ia, ctx, oracle, definition):
    import torch
    import transcode_cases as tc
    frame, main = cc.frame(), cc.container()
    name = "edit %s" % (cc.EDITS[1],)
    blobs, parts, width, height = cc.lists()[name]
    idx = [_index(ia, b, (2, 32)) for b in blobs]
    # the definition's argument errors, word for word, before anything runs
    for names, bad_parts, w, h, _, _ in cc.ARGUMENT_ERRORS:
        sources = [cc.named(n) for n in names]
        with pytest.raises(ia.MpcError) as host:
            ia.compose_container(sources, bad_parts, w, h)
        with pytest.raises(ia.MpcError) as e:
            ctx.compose(sources, None, bad_parts, w, h)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and str(e.value) == str(host.value), (names, bad_parts)
    # a context of another K: behind the header checks
    other = ia.create_compression_context(4, 8, cc.QUALITY, device=0)
    with pytest.raises(ia.MpcError) as e:
        other.compose(blobs, idx, parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "K" in str(e.value)
    with pytest.raises(ia.MpcError) as e:
        other.compose([main, b"\0" * 40], None, parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("source 1: Invalid input data")
    other.close()
    # another quantiser table
    with pytest.raises(ia.MpcError) as e:
        ctx.compose([main, cc.other_quality_container()], None, [(0, None, 0, 0), (1, (0, 0, 8, 8), 0, 0)], cc.W, cc.H)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "source 1: quantiser" in str(e.value)
    # a host-only context
    host = ia.create_compression_context(cc.K, 8, cc.QUALITY, device=-1)
    with pytest.raises(ia.MpcError) as e:
        host.compose(blobs, idx, parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host.close()
    # a busy container job slot
    tiles = region_cases.TILES_X * region_cases.TILES_Y
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, cc.K), dtype=torch.int32, device="cuda")
    ctx.container_job_begin(4, d_counts.data_ptr(), d_choices.data_ptr(), cc.W, cc.H)
    with pytest.raises(ia.MpcError) as e:
        ctx.compose(blobs, idx, parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "slot 4 is busy" in str(e.value)
    ctx.container_job_cancel(4)
    # after failed calls and after a good one the context still encodes, transcodes and composes
    view = (tc.RECTS[1], 3, 0)
    assert ctx.encode_images([frame]) == [main]
    assert ctx.compose(blobs, idx, parts, width, height, index_interval=32)[0] == definition[name]
    assert ctx.transcode_views([main], [idx[0]], [view]) == ([ia.transcode_container(main, view)], [0])
    with pytest.raises(ia.MpcError):
        ctx.compose([main, blobs[1][:len(blobs[1]) // 2]], None, parts, width, height)
    assert ctx.encode_images([frame, frame]) == [main, main]
    assert ctx.compose(blobs, None, parts, width, height) == (definition[name], None, [1, 1])
    ctx.container_job_begin(0, d_counts.data_ptr(), d_choices.data_ptr(), cc.W, cc.H)      # the slots were left idle
    ctx.container_job_cancel(0)
