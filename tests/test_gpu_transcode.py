"""Transcode on the GPU (run with -m gpu): mpc_transcode_views_indexed against its definition on the host (transcode_container),
through both routes, both flags and both index versions; against the device encoder's own container of the cropped pixels; against
the view decoder; the crop kernel on hand-made records against numpy; damaged indexes and containers; refusals; and the context
afterwards.  Every equality is exact.

The shapes are the smallest that can still go wrong: 261x277 at K = 8 is 33 x 35 = 1 155 tiles, ragged both ways, across gather block
1024, with packed and unpacked streams and both codes (region_cases.check_coverage); 1003x517 at K = 32 is eight gather blocks."""
import numpy as np
import pytest

import parse_cases
import region_cases
import transcode_cases as tc
from container_cases import FRAMES, corpus as _corpus

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
    return ia.create_compression_context(tc.K, 8, region_cases.QUALITY, device=0)


@pytest.fixture(scope="module")
def main(ia, oracle):
    region_cases.check_coverage(ia)
    return region_cases.container()


@pytest.fixture(scope="module")
def indexes(ia, main):
    """{(version, interval): index}, version 0 = none, -1 = garbage"""
    out = {(version, interval): ia.container_index(main, interval, expanded=version == 2) for version in (1, 2)
           for interval in region_cases.INTERVALS}
    out[0, 0] = None
    out[-1, 0] = b"not an index at all, whatever its length may be"
    return out


@pytest.fixture(scope="module")
def definition(ia, main):
    """{(rect, steps): transcode_container's bytes}: computed once, shared, never changed"""
    return {(rect, m): ia.transcode_container(main, (rect, m, 0)) for rect in tc.RECTS + (tc.WHOLE,) for m in tc.STEPS}


def test_device_is_the_definition(ia, ctx, main, indexes, definition):
    views = [(rect, m, 0) for rect in tc.RECTS + (tc.WHOLE,) for m in tc.STEPS]
    want = [definition[rect, m] for rect, m, _ in views]
    n = len(views)
    for (version, interval), index in indexes.items():
        route = 0 if version > 0 else 1
        for parse_all in (False, True):
            got, routes = ctx.transcode_views([main] * n, [index] * n, views, parse_all)
            assert routes == [route] * n, (version, interval, parse_all, routes)
            for g, w, view in zip(got, want, views):
                assert g == w, (version, interval, parse_all, view)


def test_eight_frames_in_one_call_and_one_per_call(ia, ctx, main, indexes, definition):
    """more frames than slots, mixing rectangles, steps, index versions, intervals and routes"""
    rects = tc.RECTS + (tc.WHOLE,)
    views = [(rects[n % len(rects)], tc.STEPS[n % len(tc.STEPS)], 0) for n in range(8)]
    keys = [(1, 32), (2, 100), (0, 0), (2, 0), (-1, 0), (1, 0), (2, 32), (1, 100)]
    want_routes = [0 if v > 0 else 1 for v, _ in keys]
    idx = [indexes[k] for k in keys]
    want = [definition[rect, m] for rect, m, _ in views]
    for parse_all in (False, True):
        together, routes = ctx.transcode_views([main] * 8, idx, views, parse_all)
        assert routes == want_routes and together == want, parse_all
        for n in range(8):
            alone, route = ctx.transcode_views([main], [idx[n]], [views[n]], parse_all)
            assert route == [want_routes[n]] and alone == [want[n]], (n, parse_all)
    backwards, routes = ctx.transcode_views([main] * 8, idx[::-1], views[::-1])
    assert routes == want_routes[::-1] and backwards == want[::-1]


def test_against_the_device_encoder(ia, ctx, main, indexes):
    frame = region_cases.frame()
    assert ctx.encode_images([frame]) == [main]
    for rect in tc.RECTS:
        x, y, w, h = rect
        fresh = ctx.encode_images([np.ascontiguousarray(frame[y:y + h, x:x + w])])
        for key in ((2, 32), (0, 0)):
            got, _ = ctx.transcode_views([main], [indexes[key]], [(rect, 0, 0)])
            assert got == fresh, (rect, key)
        for m in (1, 3):
            got, _ = ctx.transcode_views([main], [indexes[1, 32]], [(rect, m, 0)])
            assert got == [ia.truncate_container(fresh[0], m)], (rect, m)


def test_against_the_view_decoder(ia, ctx, main, indexes):
    views = [(rect, m, 0) for rect in tc.RECTS for m in (0, 1, 3)]
    n = len(views)
    for key in ((1, 32), (2, 32), (0, 0)):
        made, _ = ctx.transcode_views([main] * n, [indexes[key]] * n, views)
        pixels, _ = ctx.decode_views([main] * n, [indexes[key]] * n, views)
        for blob, want, view in zip(made, pixels, views):
            got = np.asarray(ctx.decode_images([blob])[0])
            assert got.shape == want.shape and np.array_equal(got, want), (key, view)


def test_a_fast_context_gives_the_same_bytes(ia, main, indexes, definition):
    fast = ia.create_compression_context(tc.K, 8, region_cases.QUALITY, device=0).set_fast(True)
    views = [(rect, m, 0) for rect in tc.RECTS for m in (0, 3)]
    n = len(views)
    for key in ((2, 32), (0, 0)):
        got, _ = fast.transcode_views([main] * n, [indexes[key]] * n, views)
        assert got == [definition[rect, m] for rect, m, _ in views], key
    fast.close()


def test_eight_gather_blocks(ia, oracle):
    w, h, k, _ = FRAMES[3]
    assert (w, h, k) == (1003, 517, 32) and -(-(-(-w // 8) * -(-h // 8)) // 1024) == 8
    big = ia.create_compression_context(k, 8, 3.5, device=0)
    frame = oracle.synth_frame(w, h, 103)
    blob = big.encode_images([frame])[0]
    rects = ((0, 0, 1003, 517), (496, 248, 136, 80), (992, 0, 11, 517))
    for m in (0, 5):
        views = [(rect, m, 0) for rect in rects]
        want = [ia.transcode_container(blob, view) for view in views]
        if m == 0:
            assert want[0] == blob
            assert want == big.encode_images([np.ascontiguousarray(frame[:, :1003])]) + \
                big.encode_images([np.ascontiguousarray(frame[248:328, 496:632])]) + big.encode_images([np.ascontiguousarray(frame[:, 992:])])
        for index, route in ((ia.container_index(blob, 0, expanded=True), 0), (ia.container_index(blob, 32), 0), (None, 1)):
            for parse_all in (False, True):
                got, routes = big.transcode_views([blob] * 3, [index] * 3, views, parse_all)
                assert routes == [route] * 3 and got == want, (m, route, parse_all)
    big.close()


def _framed(error, f):
    """the host definition's error as the device route words it: the same status and text behind "frame f: " """
    head = f"mpcodec status {error.status}: "
    assert str(error).startswith(head)
    return head + f"frame {f}: " + str(error)[len(head):]


def _crop_numpy(counts, choices, tiles_y, grid, m, k):
    tx0, tx1, ty0, ty1 = grid
    source = (np.arange(tx0, tx1)[:, None] * tiles_y + np.arange(ty0, ty1)[None, :]).reshape(-1)
    c = np.minimum(counts[source].astype(np.int64), m)
    live = np.arange(k)[None, None, :] < c[:, :, None]
    return c.astype(np.uint16), np.where(live, choices[source], 0).astype(np.uint32)


@pytest.mark.parametrize("k,w,h", ((3, 24, 40), (8, 261, 277)))
def test_crop_records_on_hand_made_records(ia, k, w, h):
    """random records with counts 0 ... K, and garbage in the steps at and above every count: the kernel must not carry it over"""
    import torch
    crop = ia.create_compression_context(k, 8, 3.5, device=0)
    tx, ty = -(-w // 8), -(-h // 8)
    tiles = tx * ty
    rng = np.random.default_rng([20261019, k])
    counts = rng.integers(0, k + 1, (tiles, 3)).astype(np.uint16)
    choices = rng.integers(1, 2**32, (tiles, 3, k), dtype=np.uint64).astype(np.uint32)
    d_counts = torch.from_numpy(counts.view(np.int16)).cuda()
    d_choices = torch.from_numpy(choices.view(np.int32)).cuda()
    guard = 64                                                      # words in front of and behind each output, which must stay as they are

    def run(rect, steps, dc=d_counts):
        x, y, rw, rh = rect if rect else (0, 0, w, h)
        n = (-(-(x + rw) // 8) - x // 8) * (-(-(y + rh) // 8) - y // 8)
        out_counts = torch.full((2 * guard + 3 * n,), 0x5A5A, dtype=torch.int16, device="cuda")
        out_choices = torch.full((2 * guard + 3 * n * k,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        error = None
        try:
            crop.crop_records_device(dc.data_ptr(), d_choices.data_ptr(), w, h, rect, steps, out_counts[guard:].data_ptr(),
                                     out_choices[guard:].data_ptr())
        except ia.MpcError as e:
            error = e
        torch.cuda.synchronize()
        oc, ox = out_counts.cpu().numpy().view(np.uint16), out_choices.cpu().numpy().view(np.uint32)
        assert (oc[:guard] == 0x5A5A).all() and (oc[guard + 3 * n:] == 0x5A5A).all(), (rect, steps)
        assert (ox[:guard] == 0x5A5A5A5A).all() and (ox[guard + 3 * n * k:] == 0x5A5A5A5A).all(), (rect, steps)
        return oc[guard:guard + 3 * n].reshape(n, 3), ox[guard:guard + 3 * n * k].reshape(n, 3, k), error

    corner = (8 * (tx - 2), 8 * (ty - 2), w - 8 * (tx - 2), h - 8 * (ty - 2))          # two by two tiles, ragged where the frame is
    x0 = 8 * max(tx - 5, 0)
    across = (x0, 8, w - x0, 8 * (ty - 2))                                              # the last columns but for a row at each end
    for rect in (None, (0, 0, w, h), (8, 16, 8, 8), corner, across):
        x, y, rw, rh = rect if rect else (0, 0, w, h)
        grid = (x // 8, -(-(x + rw) // 8), y // 8, -(-(y + rh) // 8))
        for steps in (0, 1, k - 1, k, k + 4):
            m = k if steps == 0 or steps > k else steps
            got_counts, got_choices, error = run(rect, steps)
            want_counts, want_choices = _crop_numpy(counts, choices, ty, grid, m, k)
            assert error is None, (rect, steps, str(error))
            assert np.array_equal(got_counts, want_counts), (rect, steps)
            assert np.array_equal(got_choices, want_choices), (rect, steps)
    if tiles > 1024:
        t0, t1, _ = region_cases.tile_range(across, h)
        assert t0 < 1024 < t1
    # a count of K + 1, inside the rectangle: used as K, the error word raised, nothing written outside the output
    bad = counts.copy()
    bad[ty + 2, 1] = k + 1
    d_bad = torch.from_numpy(bad.view(np.int16)).cuda()
    got_counts, got_choices, error = run((8, 16, 8, 8), 0, d_bad)
    assert error is not None and error.status == ia.api.MPC_ERR_BITSTREAM and str(error).endswith("Invalid bitstream")
    want_counts, want_choices = _crop_numpy(np.minimum(bad, k), choices, ty, (1, 2, 2, 3), k, k)
    assert np.array_equal(got_counts, want_counts) and np.array_equal(got_choices, want_choices)
    # ... outside the rectangle it is never looked at, and the error word was cleared by the check
    got_counts, _, error = run((0, 0, 8, 8), 0, d_bad)
    assert error is None and np.array_equal(got_counts, counts[:1])
    # arguments
    for rect in ((4, 0, 8, 8), (0, 0, 12, 8), (0, 0, w + 8, 8), (0, 0, 0, 8)):
        with pytest.raises(ia.MpcError) as e:
            crop.crop_records_device(d_counts.data_ptr(), d_choices.data_ptr(), w, h, rect, 0, d_counts.data_ptr(), d_choices.data_ptr())
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, rect
    crop.close()


def test_containers_cut_out_of_one_pursuit(ia, ctx, main, definition):
    import torch
    frame = region_cases.frame()
    w, h, k = tc.W, tc.H, tc.K
    tiles = region_cases.TILES_X * region_cases.TILES_Y
    d_rgb = torch.from_numpy(frame).cuda()
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, k), dtype=torch.int32, device="cuda")
    ctx.encode_tiles_device(d_rgb.data_ptr(), w, h, 3 * w, 0, region_cases.TILES_Y, d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    for rect in tc.RECTS[1:4]:
        for m in (0, 3):
            n = -(-rect[2] // 8) * -(-rect[3] // 8)
            out_counts = torch.zeros((n, 3), dtype=torch.int16, device="cuda")
            out_choices = torch.zeros((n, 3, k), dtype=torch.int32, device="cuda")
            ctx.crop_records_device(d_counts.data_ptr(), d_choices.data_ptr(), w, h, rect, m, out_counts.data_ptr(), out_choices.data_ptr())
            got = ctx.records_to_container_device(out_counts.data_ptr(), out_choices.data_ptr(), rect[2], rect[3])
            assert bytes(got) == definition[rect, m], (rect, m)


def test_damaged_indexes(ia, ctx, oracle, main, indexes, definition):
    other = ia.container_index(bytes(oracle.OracleContext(tc.K, 8, region_cases.QUALITY).encode_image(
        oracle.synth_frame(tc.W, tc.H, 778))), 32)
    rect, m = tc.RECTS[1], 3
    want = definition[rect, m]
    by_route = [0, 0]
    for version in (1, 2):
        damaged = parse_cases.damaged_indexes(indexes[version, 32], other, version)
        for k in range(0, len(damaged), 8):
            some = damaged[k:k + 8]
            n = len(some)
            for parse_all in (True, False):
                got, routes = ctx.transcode_views([main] * n, [bad for _, bad in some], [(rect, m, 0)] * n, parse_all)
                for g, route, (what, _) in zip(got, routes, some):
                    assert route in (0, 1), what
                    if route == 1 or parse_all:
                        assert g == want, (version, what, parse_all)
                    by_route[route] += 1
    assert by_route[0] >= 1 and by_route[1] >= 8, by_route


def test_damaged_containers(ia, ctx, oracle):
    """a slice of the corpus, the containers of this context's K: the host definition's status and text, behind "frame N: " """
    seen = set()
    for n, blob, xs in _corpus(oracle):
        if FRAMES[n][2] != tc.K:
            continue
        index = ia.container_index(blob, 32, expanded=True)
        for k, x in list(enumerate(xs))[::4]:
            for view in ((tc.WHOLE, 0, 0), ((0, 0, 8, 8), 1, 0)):
                try:
                    want = ia.transcode_container(x, view)
                    if ia.container_info(x)[2:] != (tc.K, 8):       # the definition takes any K and block size, a context its own
                        want = ia.api.MPC_ERR_ARGUMENT
                except ia.MpcError as e:
                    want = e
                for idx in (None, index):
                    if want == ia.api.MPC_ERR_ARGUMENT:
                        with pytest.raises(ia.MpcError) as e:
                            ctx.transcode_views([blob, x], [index, idx], [(tc.WHOLE, 0, 0), view], True)
                        assert e.value.status == want and ": frame 1: " in str(e.value), (n, k, view, str(e.value))
                    elif isinstance(want, ia.MpcError):
                        with pytest.raises(ia.MpcError) as e:
                            ctx.transcode_views([blob, x], [index, idx], [(tc.WHOLE, 0, 0), view], True)
                        assert e.value.status == want.status and str(e.value) == _framed(want, 1), (n, k, view, str(e.value), str(want))
                        seen.add((want.status, str(want).split(": ", 1)[1]))
                    else:
                        got, routes = ctx.transcode_views([blob, x], [index, idx], [(tc.WHOLE, 0, 0), view], True)
                        assert got == [blob, want], (n, k, view)
    assert (ia.api.MPC_ERR_BITSTREAM, "Invalid input data") in seen, seen


def test_a_length_above_k(ia, ctx, main, indexes):
    s = ia.read_compressed(main)
    lengths = s["lengths"].copy()
    lengths[int(np.flatnonzero(lengths == tc.K)[0])] = tc.K + 1
    bad = ia.write_compressed(s["W"], s["H"], s["K"], s["bs"], s["quant"].astype(np.float64), lengths, s["codes"])
    for index in (None, ia.container_index(bad, 32), ia.container_index(bad, 32, expanded=True)):
        for view in ((tc.WHOLE, 1, 0), ((0, 0, 8, 8), 0, 0)):
            for parse_all in (False, True):
                with pytest.raises(ia.MpcError) as e:
                    ctx.transcode_views([bad], [index], [view], parse_all)
                assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith(": frame 0: Invalid bitstream"), (view, parse_all)


def test_refusals_and_the_context_afterwards(ia, ctx, oracle, main, indexes, definition):
    import torch
    frame = region_cases.frame()
    view = (tc.RECTS[1], 3, 0)
    want = definition[tc.RECTS[1], 3]
    # argument errors name the frame and come before anything runs
    for bad in tc.ARGUMENT_ERRORS:
        for index in (indexes[2, 32], None):
            with pytest.raises(ia.MpcError) as e:
                ctx.transcode_views([main, main], [index, index], [view, bad])
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "frame 1: " in str(e.value), bad
            try:
                ia.transcode_container(main, bad)
            except ia.MpcError as host:
                assert str(e.value) == _framed(host, 1), bad
    # a context of another K
    other = ia.create_compression_context(4, 8, region_cases.QUALITY, device=0)
    for index in (indexes[1, 32], None):
        with pytest.raises(ia.MpcError) as e:
            other.transcode_views([main], [index], [view])
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "K" in str(e.value)
    other.close()
    # a host-only context
    host = ia.create_compression_context(tc.K, 8, region_cases.QUALITY, device=-1)
    with pytest.raises(ia.MpcError) as e:
        host.transcode_views([main], [indexes[1, 32]], [view])
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host.close()
    # a busy container job slot
    tiles = region_cases.TILES_X * region_cases.TILES_Y
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, tc.K), dtype=torch.int32, device="cuda")
    ctx.container_job_begin(4, d_counts.data_ptr(), d_choices.data_ptr(), tc.W, tc.H)
    with pytest.raises(ia.MpcError) as e:
        ctx.transcode_views([main], [indexes[1, 32]], [view])
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "slot 4 is busy" in str(e.value)
    ctx.container_job_cancel(4)
    # after failed calls and after a good one the context still encodes and transcodes
    assert ctx.encode_images([frame]) == [main]
    assert ctx.transcode_views([main] * 2, [indexes[2, 0], None], [view] * 2) == ([want] * 2, [0, 1])
    with pytest.raises(ia.MpcError):
        ctx.transcode_views([main, main[:len(main) // 2]], [None, None], [view, (tc.WHOLE, 0, 0)])
    assert ctx.encode_images([frame, frame]) == [main, main]
    assert ctx.transcode_views([main], [indexes[1, 100]], [view]) == ([want], [0])
    ctx.container_job_begin(0, d_counts.data_ptr(), d_choices.data_ptr(), tc.W, tc.H)      # the slots were left idle
    ctx.container_job_cancel(0)
