"""The delta encoder's change tolerance on the GPU (run with -m gpu): mp_tile_diff_tol_kernel against the host definition through
mpc_tile_diff_tolerance_device on every case of tests/tolerance_cases.py, and sessions with a tolerance against the numpy replay: the
list, the composite, the held totals, the container (encode_image of the composite), the patch stream and the budgeted stream.  Every
equality is exact.  K = 8.

The shapes are tolerance_cases.SHAPES: 8x8 and 5x3 are one tile; 531x29 is 67 x 4 tiles -- two strips of 64, a last tile row of 5 pixel
rows, an odd 3 * width (the byte path); 528x32 takes the 8-byte path over 66 tiles; 1040x72 is 1170 tiles: three strips, two list
blocks."""
import ctypes as C

import numpy as np
import pytest

import delta_cases as dc
import rate_cases as rc
import stream_order as so
import tolerance_cases as tc

pytestmark = pytest.mark.gpu

K = tc.K


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def ctx(ia):
    c = ia.create_compression_context(K, 8, dc.QUALITY, device=0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cases' own arrays stay as they are


def _tiles(name):
    return tc.grid(name)[0] * tc.grid(name)[1]


_WANT = {}


def _want(ctx, px):
    """encode_image of a frame, once per frame"""
    key = np.asarray(px).tobytes()
    if key not in _WANT:
        _WANT[key] = ctx.encode_image(np.ascontiguousarray(px))
    return _WANT[key]


_REPLAY = {}


def _replay(label, tolerances=None):
    """the numpy replay of a sequence, once, shared and never changed"""
    frames, T, name = tc.sequence(label)
    key = (label, None if tolerances is None else tuple(tolerances))
    if key not in _REPLAY:
        _REPLAY[key] = tc.replay(frames, T if tolerances is None else list(tolerances))
    return frames, T, name, _REPLAY[key]


def _diff(ctx, a, b, T, with_sse=True, entry="tolerance"):
    """one launch -> (list, count words, sse or None, kept afterwards, the frame's buffer afterwards)"""
    import torch
    tiles = dc.grid(b.w, b.h)[0] * dc.grid(b.w, b.h)[1]
    kept, cur = _dev(a.pixels), _dev(b.raw)
    d_list = torch.full((tiles + 1,), -1, dtype=torch.int32, device="cuda")
    d_count = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    d_sse = torch.full((tiles + 1,), -1, dtype=torch.int32, device="cuda")
    if entry == "tolerance":
        ctx.tile_diff_tolerance_device(kept.data_ptr(), cur.data_ptr() + b.off, b.w, b.h, b.stride, T, d_list.data_ptr(), d_count.data_ptr(),
                                       d_sse.data_ptr() if with_sse else 0)
    else:
        ctx.tile_diff_device(kept.data_ptr(), cur.data_ptr() + b.off, b.w, b.h, b.stride, d_list.data_ptr(), d_count.data_ptr())
    torch.cuda.synchronize()
    return (d_list.cpu().numpy(), d_count.cpu().numpy(), d_sse.cpu().numpy().view(np.uint32), kept.cpu().numpy(), cur.cpu().numpy())


# ---- 1. the kernel against the host definition ----
@pytest.mark.parametrize("kind", tc.STRIDES)
@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_the_kernel_is_the_host_definition(ia, ctx, name, kind):
    w, h = tc.SHAPES[name]
    tiles = _tiles(name)
    word_path = 0
    for lead in (0, 1):
        for label, a, b, T in tc.tile_cases(name, kind, lead):
            want_list, want_sse, want_comp = ia.changed_tiles_tolerance(a.pixels, b.pixels, T)
            model = tc.diff(a, b, T)
            assert all(np.array_equal(x, y) for x, y in zip(model, (want_list, want_sse, want_comp))), (name, label)
            word_path += (b.off % 8 == 0 and b.stride % 8 == 0 and (3 * w) % 8 == 0)
            for with_sse in (True, False):
                got, n, sse, kept, cur = _diff(ctx, a, b, T, with_sse)
                assert n[0] == want_list.size and n[1] == -1, (name, lead, label, n)
                assert (got[:want_list.size] == want_list).all() and (got[want_list.size:] == -1).all(), (name, lead, label)
                if with_sse:
                    assert (sse[:tiles] == want_sse).all() and sse[tiles] == 0xffffffff, (name, lead, label)
                else:
                    assert (sse == 0xffffffff).all()
                assert (kept == want_comp).all(), (name, lead, label)              # the kept copy is the composite
                assert (cur == b.raw).all()                                        # and the new frame is only read
    assert (word_path > 0) == ((3 * w) % 8 == 0 and kind != "odd")                 # both fetch paths where the shape has both


# ---- 2. tolerance 0 is the diff there was ----
@pytest.mark.parametrize("name", ["tiny", "ragged2", "word2", "blocks"])
def test_tolerance_0_is_the_plain_diff(ia, ctx, name):
    for kind in tc.STRIDES:
        for label, a, b, _ in tc.tile_cases(name, kind):
            new = _diff(ctx, a, b, 0)
            old = _diff(ctx, a, b, 0, entry="plain")
            assert (new[0] == old[0]).all() and (new[1] == old[1]).all() and (new[3] == old[3]).all(), (name, label)
            assert (new[3] == b.pixels).all()


# ---- 3. the stream contract ----
def test_ordered_on_the_callers_stream(ia, ctx):
    """stream_order.behind_delay, as tests/test_gpu_stream_order.py drives mpc_tile_diff_device: behind a delay on a side stream the
    inputs turn from B into A; the consumer behind the call must see A's result, and the call must return while the delay runs"""
    import torch
    name, T = "ragged2", 100
    cases = {label.split(" ", 1)[1]: (a, b) for label, a, b, _ in tc.tile_cases(name, "tight")}
    (ka, ca), (kb, cb) = cases["cross"], cases["noise"]
    w, h = tc.SHAPES[name]
    tiles = _tiles(name)
    want_list, want_sse, want_comp = ia.changed_tiles_tolerance(ka.pixels, ca.pixels, T)
    other = ia.changed_tiles_tolerance(kb.pixels, cb.pixels, T)
    assert 0 < want_list.size < tiles and other[0].size != want_list.size
    lst = np.full(tiles, so.POISON * 0x01010101, np.int32)
    lst[:want_list.size] = want_list
    S = torch.cuda.Stream()
    cpm = so.cycles_per_ms(torch)

    def call(b):
        ctx.tile_diff_tolerance_device(b.ptr("kept"), b.ptr("rgb"), w, h, 0, T, b.ptr("list"), b.ptr("count"), b.ptr("sse"), stream=b.stream)
        b.probe()
    inputs = {"kept": (np.array(ka.pixels), np.array(kb.pixels)), "rgb": (np.array(ca.pixels), np.array(cb.pixels))}
    want = {"kept": want_comp, "list": lst, "count": np.array([want_list.size], np.int32), "sse": want_sse}
    _, _, warm = so.behind_delay(torch, S, call, inputs, want, 1000)
    got, _, info = so.behind_delay(torch, S, call, inputs, want, so.delay_ms_for(warm["host_ms"]) * cpm)
    for key, value in want.items():
        assert np.array_equal(got[key].reshape(value.shape), value), key
    assert info["running"], "mpc_tile_diff_tolerance_device returned only after the stream had drained"
    # the control: told the null stream it runs at once, on B, and the consumer does not see A's list
    got, _, _ = so.behind_delay(torch, S, call, inputs, want, so.delay_ms_for(warm["host_ms"]) * cpm, lib_stream=0)
    assert not np.array_equal(got["count"], want["count"])


# ---- 4. sessions ----
def _check_call(ia, ctx, enc, r, blob, label, i):
    tiles = dc.grid(r["composite"].shape[1], r["composite"].shape[0])[0] * dc.grid(r["composite"].shape[1], r["composite"].shape[0])[1]
    assert enc.info == (tiles, len(r["list"]), r["key"]), (label, i, enc.info)
    assert np.array_equal(enc.changed(), r["list"]), (label, i)
    assert np.array_equal(enc.frame(), r["composite"]), (label, i)
    assert enc.held() == (r["held"], r["held_sse"]), (label, i, enc.held())
    assert blob == _want(ctx, r["composite"]), (label, i)


@pytest.mark.parametrize("pixels", ["host", "device"])
@pytest.mark.parametrize("label", list(tc.SEQUENCES))
def test_a_tolerant_session(ia, ctx, label, pixels):
    import torch
    frames, T, name, calls = _replay(label)
    w, h = tc.SHAPES[name]
    enc = ctx.delta_encoder(w, h)
    assert enc.tolerance == 0
    enc.set_tolerance(T)
    assert enc.tolerance == T
    for i, (px, r) in enumerate(zip(frames, calls)):
        interval = 32 if i % 3 == 1 else None
        if pixels == "host":
            got = enc.encode(dc.Layout(px, tc.STRIDES[i % 3], 0, 70 + i).pixels, index_interval=interval)
        else:
            lay = dc.Layout(px, tc.STRIDES[(i + 1) % 3], i % 2, 80 + i)
            d_raw = _dev(lay.raw)
            got = enc.encode_device(d_raw.data_ptr() + lay.off, lay.stride, index_interval=interval)
            assert (d_raw.cpu().numpy() == lay.raw).all()
        blob = got if interval is None else got[0]
        _check_call(ia, ctx, enc, r, blob, label, i)
        if interval is not None:
            assert got[1] == ia.container_index(blob, interval, expanded=True), (label, i)
        # the session's own buffer is the composite too: read through the plain diff, which copies what differs from a kept copy of
        # another value in every byte
        seen = torch.full((h, w, 3), 255, dtype=torch.uint8, device="cuda")
        d_list, d_count = torch.zeros(_tiles(name), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        assert r["composite"].max() < 255 and enc.frame_device()
        ctx.tile_diff_device(seen.data_ptr(), enc.frame_device(), w, h, 0, d_list.data_ptr(), d_count.data_ptr())
        torch.cuda.synchronize()
        assert (seen.cpu().numpy() == r["composite"]).all() and d_count.item() == _tiles(name), (label, i)
        # held_sse is the composite's squared error against the frame
        assert enc.held()[1] == int(((r["composite"].astype(np.int64) - px) ** 2).sum()), (label, i)
    assert sum(r["held"] for r in calls) > 0 and any(0 < len(r["list"]) < _tiles(name) for r in calls)
    enc.close()


# ---- 5. set_tolerance(0) changes nothing ----
@pytest.mark.parametrize("label", ["noise ragged2", "ramp word2"])
def test_tolerance_0_is_an_untouched_session(ia, ctx, label):
    frames, _, name = tc.sequence(label)
    w, h = tc.SHAPES[name]
    a, b = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
    a.set_tolerance(0)
    for i, px in enumerate(frames):
        assert a.encode(px, index_interval=0) == b.encode(px, index_interval=0), (label, i)
        assert a.info == b.info and np.array_equal(a.changed(), b.changed()) and a.held() == (0, 0) == b.held()
        assert a.info[1] == (dc.changed_tiles(frames[i - 1], px).size if i else _tiles(name))
        assert np.array_equal(a.frame(), px) and np.array_equal(b.frame(), px)
    a.close()
    b.close()


# ---- 6. the tolerance moves between calls ----
def test_the_tolerance_is_raised_and_lowered(ia, ctx):
    label = "noise ragged2"
    frames, T, name = tc.sequence(label)
    tolerances = [T, T, 4 * T, 0, T // 2, tc.MAX_SSE, 1][:len(frames)]
    _, _, _, calls = _replay(label, tolerances)
    w, h = tc.SHAPES[name]
    enc = ctx.delta_encoder(w, h)
    counts = []
    for i, (px, r) in enumerate(zip(frames, calls)):
        enc.set_tolerance(tolerances[i])
        blob = enc.encode(px)
        assert enc.info[2] == int(i == 0)                                          # no key frame but the first
        _check_call(ia, ctx, enc, r, blob, label, i)
        counts.append(enc.info[1])
    assert len(set(counts[1:])) > 2 and calls[5]["list"].size == 0 and calls[3]["held"] == 0
    enc.close()


# ---- 7. the patch stream ----
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("label", ["noise blocks", "ramp ragged2"])
def test_a_tolerant_patch_stream(ia, ctx, label, indexed):
    frames, T, name, calls = _replay(label)
    w, h = tc.SHAPES[name]
    enc, dec = ctx.delta_encoder(w, h), ctx.patch_decoder(w, h)
    enc.set_tolerance(T)
    for i, (px, r) in enumerate(zip(frames, calls)):
        patch = enc.encode_patch(px, index_interval=0, index_min_bytes=0) if indexed else enc.encode_patch(px)
        assert np.array_equal(enc.changed(), r["list"]) and enc.held() == (r["held"], r["held_sse"]), (label, i)
        assert np.array_equal(enc.frame(), r["composite"]), (label, i)
        info = ia.patch_info(patch)
        assert info["sequence"] == i and info["key"] == r["key"], (label, i, info)
        dec.apply(patch)
        assert (dec.frame() == ctx.decode_images([_want(ctx, r["composite"])])[0]).all(), (label, i)     # the twin invariant, on C_n
    enc.close()
    dec.close()


# ---- 8. the budgeted stream ----
@pytest.mark.parametrize("label", ["noise ragged2", "ramp word2"])
def test_an_unlimited_budget_gives_the_tolerant_patches(ia, ctx, label):
    frames, T, name, calls = _replay(label)
    w, h = tc.SHAPES[name]
    a, b = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
    a.set_tolerance(T)
    b.set_tolerance(T)
    for i, (px, r) in enumerate(zip(frames, calls)):
        got, info = a.encode_patch_budget(px, 1 << 40)
        assert got == b.encode_patch(px), (label, i)
        assert np.array_equal(a.changed(), r["list"]) and a.held() == b.held() == (r["held"], r["held_sse"])
        assert info.changed == len(r["list"]) and info.owed == 0 and (a.sent() == K).all()
    a.close()
    b.close()


@pytest.mark.parametrize("label", ["noise ragged2"])
def test_a_tight_budget_is_the_replay_on_the_composites(ia, ctx, label):
    """rate_cases.Replay fed C_n in place of frame n: its changed tiles are then the tolerant list, and its patches, its sent map and
    the receiver's frame must be the session's.  The budget is half the largest non-key patch of the uncut stream, raised to
    size(255) + 1 of every call where that is more (rate_cases.tight_stream's rule)."""
    from test_gpu_rate import DevicePieces
    frames, T, name, calls = _replay(label)
    w, h = tc.SHAPES[name]
    composites = [r["composite"] for r in calls]
    pieces = DevicePieces(ia, ctx, name)
    loose = rc.Replay(pieces, w, h, K)
    uncut = [loose.call(c, 1 << 40) for c in composites]
    for i, (u, r) in enumerate(zip(uncut, calls)):
        assert u["changed"] == len(r["list"]), i                                    # the composites' plain diff is the tolerant diff
    budget = max(u["all_bytes"] for u in uncut[1:]) // 2
    for _ in range(8):
        replay, results = rc.Replay(pieces, w, h, K), []
        for c in composites:
            r = replay.call(c, budget)
            need = (replay.refused_size255 if r is None else r["size255"]) + 1
            if need > budget:
                budget = need
                break
            results.append(r)
        else:
            break
    assert len(results) == len(composites) and any(r["lambda_index"] >= 0 for r in results)
    enc, dec = ctx.delta_encoder(w, h), ctx.patch_decoder(w, h)
    enc.set_tolerance(T)
    header_quant = None
    for i, (px, r, c) in enumerate(zip(frames, results, calls)):
        patch, info = enc.encode_patch_budget(px, budget)
        assert len(patch) <= budget and patch == r["patch"], (label, i, info)
        assert (enc.sent() == r["sent"]).all() and np.array_equal(enc.changed(), c["list"]) and enc.held() == (c["held"], c["held_sse"])
        for field in ("changed", "candidates", "sent_tiles", "owed", "lambda_index", "probes", "all_bytes", "key"):
            assert getattr(info, field) == r[field], (label, i, field)
        dec.apply(patch)
        if header_quant is None:
            header_quant = ia.read_compressed(patch[ia.patch_info(patch)["container_offset"]:])["quant"]
        assert (dec.frame() == pieces.decode_cut(c["composite"], enc.sent(), header_quant)).all(), (label, i)
    enc.close()
    dec.close()


# ---- 9. refusals ----
def test_refusals(ia, ctx):
    import torch
    L = ctx.L
    A = ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_delta_set_tolerance(None, 7) == A
    w, h = tc.SHAPES["ragged2"]
    tiles = _tiles("ragged2")
    # the device entry point: null pointers and bad strides, with nothing enqueued
    kept = torch.full((h, w, 3), 5, dtype=torch.uint8, device="cuda")
    cur = torch.full((h, w, 3), 9, dtype=torch.uint8, device="cuda")
    d_list, d_count = torch.full((tiles,), -1, dtype=torch.int32, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
    good = dict(kept=kept.data_ptr(), cur=cur.data_ptr(), w=w, h=h, stride=0, list=d_list.data_ptr(), count=d_count.data_ptr())
    for bad in (dict(kept=None), dict(cur=None), dict(list=None), dict(count=None), dict(stride=3 * w - 1), dict(stride=1), dict(w=0), dict(h=0)):
        v = dict(good, **bad)
        assert L.mpc_tile_diff_tolerance_device(ctx.h, v["kept"], v["cur"], v["w"], v["h"], v["stride"], 10, v["list"], v["count"], None, None) == A, bad
    assert L.mpc_tile_diff_tolerance_device(None, good["kept"], good["cur"], w, h, 0, 10, good["list"], good["count"], None, None) == A
    torch.cuda.synchronize()
    assert (kept == 5).all() and (d_list == -1).all() and (d_count == -1).all()
    host_only = ia.create_compression_context(K, 8, dc.QUALITY, device=-1)
    assert L.mpc_tile_diff_tolerance_device(host_only.h, good["kept"], good["cur"], w, h, 0, 10, good["list"], good["count"], None, None) == \
        ia.api.MPC_ERR_NO_DEVICE
    host_only.close()
    # a refused encode call leaves the tolerance, the composite and the held totals as they were
    frames, T, name, calls = _replay("noise ragged2")
    enc = ctx.delta_encoder(w, h)
    with pytest.raises(ia.MpcError) as e:
        enc.frame()                                                                # no call yet: no frame
    assert e.value.status == A
    enc.set_tolerance(T)
    for px in frames[:3]:
        enc.encode(px)
    before = (enc.tolerance, enc.frame(), enc.held(), enc.changed().copy(), enc.info)
    assert before[2] == (calls[2]["held"], calls[2]["held_sse"]) and before[2][0] > 0
    out, n, info = C.POINTER(C.c_uint8)(), C.c_size_t(7), ia.api.MpcDeltaInfo(-1, -1, -1)
    px = np.ascontiguousarray(frames[3])
    for stride, flags, rgb in ((3 * w - 1, 0, px.ctypes.data), (0, 64, px.ctypes.data), (0, 0, None)):
        assert L.mpc_delta_encode(enc.h, rgb, stride, None, flags, -1, C.byref(out), C.byref(n), None, None, C.byref(info)) == A
    assert L.mpc_delta_frame(enc.h, px.ctypes.data, 3 * w - 1) == A
    after = (enc.tolerance, enc.frame(), enc.held(), enc.changed().copy(), enc.info)
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2] == after[2] and (before[3] == after[3]).all() and before[4] == after[4]
    blob = enc.encode(frames[3])                                                   # still a delta, and the model's
    _check_call(ia, ctx, enc, calls[3], blob, "after the refusals", 3)
    enc.close()
