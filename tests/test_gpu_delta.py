"""The delta encoder on the GPU (run with -m gpu): each of its three kernels alone against the numpy model of tests/delta_cases.py
through the *_device entry points, and sessions: after every call the container is byte for byte encode_image of that frame and the
list is the model's, whatever came before.  Every equality is exact.

The shapes are the smallest that can still go wrong (delta_cases.SHAPES): 83x45 is 11 x 6 tiles, ragged both ways; 8x8 and 5x3 are one
tile; 16x16 at K = 32 with the all-ones table has full-length records; 200x136 is 425 tiles: more than 64 (a second packed column),
424 of them pack 7 columns with the last one partial.  3 * width is a multiple of 8 for 8, 16 and 200 (the 8-byte path where the
stride and the base allow it) and is not for 83 and 5."""
import ctypes as C

import numpy as np
import pytest

import delta_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def ctxs(ia):
    made = {K: ia.create_compression_context(K, 8, dc.QUALITY, device=0) for K in (8, 32)}
    yield made
    for c in made.values():
        c.close()


_WANT = {}


def _want(ctx, name, px, quant="shape"):
    """encode_image of the frame: computed once per (shape, flavour, table, pixels), shared, never changed"""
    q = dc.quant(name) if isinstance(quant, str) else quant
    key = (name, ctx.fast, None if q is None else np.asarray(q).tobytes(), np.asarray(px).tobytes())
    if key not in _WANT:
        _WANT[key] = ctx.encode_image(np.ascontiguousarray(px), quant=q)
    return _WANT[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cases' own arrays stay as they are


def _ctx(ctxs, name):
    return ctxs[dc.SHAPES[name][2]]


# ---- each kernel alone ----
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_diff_kernel(ia, ctxs, name):
    import torch
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = dc.grid(w, h)[0] * dc.grid(w, h)[1]
    word_path = 0
    for lead in (0, 1):
        for label, a, b in dc.diff_pairs(name, lead):
            kept, cur = _dev(a.pixels), _dev(b.raw)
            d_list, d_count = torch.full((tiles + 1,), -1, dtype=torch.int32, device="cuda"), torch.full((2,), -1, dtype=torch.int32, device="cuda")
            assert kept.data_ptr() % 8 == 0 and cur.data_ptr() % 8 == 0
            word_path += (cur.data_ptr() + b.off) % 8 == 0 and b.stride % 8 == 0 and (3 * w) % 8 == 0
            ctx.tile_diff_device(kept.data_ptr(), cur.data_ptr() + b.off, w, h, b.stride, d_list.data_ptr(), d_count.data_ptr())
            torch.cuda.synchronize()
            want = dc.expected(a, b)
            got, n = d_list.cpu().numpy(), d_count.cpu().numpy()
            assert n[0] == want.size and n[1] == -1, (name, lead, label, n)
            assert (got[:want.size] == want).all() and (got[want.size:] == -1).all(), (name, lead, label)
            assert (kept.cpu().numpy() == b.pixels).all(), (name, lead, label)     # the kept copy is the new frame
            assert (cur.cpu().numpy() == b.raw).all()                              # and the new frame is only read
    assert (word_path > 0) == ((3 * w) % 8 == 0)                                   # both fetch paths where the shape has both
    # row_stride 0 is the tight stride
    px = dc.frame(w, h, 11)
    kept, cur = _dev(px), _dev(dc.bump(px, w - 1, h - 1, 2))
    d_list, d_count = torch.zeros(tiles, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.tile_diff_device(kept.data_ptr(), cur.data_ptr(), w, h, 0, d_list.data_ptr(), d_count.data_ptr())
    torch.cuda.synchronize()
    assert d_count.item() == 1 and d_list[0].item() == tiles - 1


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_pack_kernel(ia, ctxs, name):
    import torch
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = dc.grid(w, h)[0] * dc.grid(w, h)[1]
    cases = dc.pack_cases(name)
    cases.append(("an entry outside the frame", cases[0][1], [0, tiles, -1, tiles - 1], 3))
    for c, (label, px, listed, rows) in enumerate(cases):
        kind, lead = dc.STRIDES[c % 3], (c // 3) % 2
        lay = dc.Layout(px, kind, lead, 300 + c)
        src = _dev(lay.raw)
        n = len(listed)
        R, Cc, stride, nbytes = ia.delta_pack_geometry(n, rows)
        assert (R, Cc, stride, nbytes) == dc.pack_geometry(n, rows)
        pad = 16 * (c % 2)                                                         # a packed stride above the minimum: the rest untouched
        packed = torch.full((8 * R, stride + pad), 0xA5, dtype=torch.uint8, device="cuda")
        d_list = _dev(np.asarray(listed, np.int32))
        ctx.pack_tiles_device(src.data_ptr() + lead, w, h, lay.stride, d_list.data_ptr(), n, rows, packed.data_ptr(), stride + pad if pad else 0)
        torch.cuda.synchronize()
        got = packed.cpu().numpy()
        assert (got[:, :stride].reshape(8 * R, 8 * Cc, 3) == dc.pack(px, listed, rows)).all(), (name, label, kind, lead)
        assert (got[:, stride:] == 0xA5).all() and (src.cpu().numpy() == lay.raw).all()
    with pytest.raises(ia.MpcError) as e:                                          # a packed stride that is no multiple of 8
        ctx.pack_tiles_device(src.data_ptr(), w, h, 0, d_list.data_ptr(), 1, 64, packed.data_ptr(), 28)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT


def test_scatter_kernel(ia, ctxs):
    import torch
    for K, tiles, listed in ((8, 66, [5, 0, 65, 17]), (32, 4, [3]), (8, 425, list(range(424, -1, -3))), (8, 66, [5, 66, 0, -1, 64])):
        ctx = ctxs[K]
        pc, pch = dc.records(len(listed), K, 1)
        counts, choices = dc.records(tiles, K, 2)
        want_c, want_r, bad = dc.scatter(pc, pch, listed, counts, choices)
        d = [_dev(x) for x in (pc, pch, np.asarray(listed, np.int32), counts, choices)]
        args = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(listed), d[3].data_ptr(), d[4].data_ptr(), tiles)
        if bad:                                                                    # the entry is skipped and the error word set
            with pytest.raises(ia.MpcError) as e:
                ctx.scatter_records_device(*args)
            assert e.value.status == ia.api.MPC_ERR_BITSTREAM
            assert ctx.L.mpc_crop_records_check(ctx.h, None) == ia.api.MPC_OK      # read and cleared
        else:
            ctx.scatter_records_device(*args)
        torch.cuda.synchronize()
        assert (d[3].cpu().numpy() == want_c).all() and (d[4].cpu().numpy() == want_r).all(), (K, tiles, bad)
        assert (d[0].cpu().numpy() == pc).all() and (d[1].cpu().numpy() == pch).all()


# ---- sessions ----
def _all(name):
    w, h, _ = dc.SHAPES[name]
    return dc.grid(w, h)[0] * dc.grid(w, h)[1]


def _step(enc, ctx, name, px, want_changed, is_key=0, **kw):
    """one call: the bytes are encode_image's, the list and the info are the model's"""
    quant = kw.pop("quant", dc.quant(name))
    got = enc.encode(px, quant=quant, **kw)
    assert got == _want(ctx, name, px, quant), (name, enc.info)
    tiles = _all(name)
    want = np.arange(tiles) if is_key else np.asarray(want_changed)
    assert enc.info == (tiles, want.size, is_key), (name, enc.info, want.size)
    assert (enc.changed() == want).all() and enc.changed().size == want.size
    return got


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_a_sequence(ia, ctxs, oracle, name):
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    frames = dc.sequence(name)
    octx = oracle.OracleContext(K, 8, dc.QUALITY) if name in ("ragged", "full", "tiny") else None
    enc = ctx.delta_encoder(w, h)
    for i, px in enumerate(frames):
        got = _step(enc, ctx, name, px, dc.changed_tiles(frames[i - 1], px) if i else None, is_key=int(i == 0))
        if octx:
            assert got == octx.encode_image(px, quant=dc.quant(name)), (name, i)
    assert any(0 < dc.changed_tiles(a, b).size < _all(name) for a, b in zip(frames, frames[1:])) or _all(name) == 1
    enc.close()


def test_single_changes_and_none(ia, ctxs):
    name = "ragged"
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tx, ty = dc.grid(w, h)
    px = np.array(dc.frame(w, h, 21))
    enc = ctx.delta_encoder(w, h)
    first = _step(enc, ctx, name, px, None, is_key=1)
    # the identical frame: nothing changed, the same bytes, no pursuit launched
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    assert _step(enc, ctx, name, px, []) == first
    assert ctx.read_kernel_timing()[1] == 0
    # one byte by one: in an interior tile, in tile 0, at pixel (w - 1, h - 1) of the ragged corner tile
    for x, y, c in ((43, 20, 1), (0, 0, 0), (w - 1, h - 1, 2)):
        px = dc.bump(px, x, y, c)
        _step(enc, ctx, name, px, [(x // 8) * ty + y // 8])
        assert ctx.read_kernel_timing()[1] > 0                                     # of one packed tile
    ctx.kernel_timing(False)
    # the stride padding alone changes: nothing changed
    a, b = dc.Layout(px, "odd", 0, 1), dc.Layout(px, "odd", 0, 2)
    assert (a.raw != b.raw).any() and (a.pixels == b.pixels).all()
    _step(enc, ctx, name, a.pixels, [])
    _step(enc, ctx, name, b.pixels, [])
    # a checkerboard, then back: A -> B -> A returns A's bytes
    board = dc.tile_sets(name)["checkerboard"]
    _step(enc, ctx, name, dc.change_tiles(px, board, 9), board)
    assert _step(enc, ctx, name, px, board) == _want(ctx, name, px)
    enc.close()


def test_packed_columns(ia, ctxs):
    """425 tiles: all but one (7 packed columns, the last one partial), exactly 64 and exactly 65 changed tiles"""
    name = "many"
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    sets = dc.tile_sets(name)
    assert len(sets["all but one"]) == 424 and len(sets["64"]) == 64 and len(sets["65"]) == 65
    px = np.array(dc.frame(w, h, 31))
    enc = ctx.delta_encoder(w, h)
    _step(enc, ctx, name, px, None, is_key=1)
    for i, label in enumerate(("all but one", "64", "65", "checkerboard", "all")):
        px = dc.change_tiles(px, sets[label], 40 + i)
        _step(enc, ctx, name, px, sets[label])
    enc.close()


def test_key_frames(ia, ctxs):
    name = "ragged"
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    a, b = np.array(dc.frame(w, h, 51)), dc.change_tiles(dc.frame(w, h, 51), [3, 40], 1)
    enc = ctx.delta_encoder(w, h)
    direct = _step(enc, ctx, name, a, None, is_key=1)
    _step(enc, ctx, name, b, [3, 40])
    _step(enc, ctx, name, b, None, is_key=1, key=True)                         # MPC_DELTA_KEY
    # MPC_DELTA_PACK_ALWAYS on a key frame: list -> pack -> encode -> scatter of every tile equals the direct key frame
    assert enc.encode(a, key=True, pack_always=True) == direct and enc.info == (66, 66, 1) and enc.changed().size == 66
    other = ctx.delta_encoder(w, h)
    assert other.encode(a, pack_always=True) == direct and other.info == (66, 66, 1)
    other.close()
    # the quantiser table changes between calls: a key frame, with the new table's bytes; the same table again is a delta
    table = ia.quant_tables(K, 5.0)
    assert _step(enc, ctx, name, a, None, is_key=1, quant=table) != direct
    _step(enc, ctx, name, b, [3, 40], quant=table)
    _step(enc, ctx, name, b, None, is_key=1, quant=None)                              # NULL: the context's tables as they are now
    _step(enc, ctx, name, a, [3, 40], quant=ctx.quant)                             # ... which these are
    # the fast flag toggles between calls: a key frame, and the bytes are the fast encode
    try:
        ctx.set_fast(True)
        fast = _step(enc, ctx, name, a, None, is_key=1)
        assert fast == ctx.encode_image(a) and enc.info[2] == 1
        _step(enc, ctx, name, b, [3, 40])
        # a whole sequence on a fast context
        seq = ctx.delta_encoder(w, h)
        frames = dc.sequence(name)
        for i, px in enumerate(frames):
            _step(seq, ctx, name, px, dc.changed_tiles(frames[i - 1], px) if i else None, is_key=int(i == 0))
        seq.close()
    finally:
        ctx.set_fast(False)
    _step(enc, ctx, name, b, None, is_key=1)
    enc.close()


def test_the_index_comes_with_the_container(ia, ctxs):
    name = "many"
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    frames = dc.sequence(name, 3)
    enc = ctx.delta_encoder(w, h)
    for i, px in enumerate(frames):
        for interval in (0, 32):
            blob, index = enc.encode(px, index_interval=interval)
            assert blob == _want(ctx, name, px) and index == ia.container_index(blob, interval, expanded=True), (i, interval)
    enc.close()


def test_refusals_leave_the_session_valid(ia, ctxs):
    import torch
    name = "ragged"
    ctx = _ctx(ctxs, name)
    L = ctx.L
    w, h, K = dc.SHAPES[name]
    a = np.array(dc.frame(w, h, 61))
    enc = ctx.delta_encoder(w, h)
    _step(enc, ctx, name, a, None, is_key=1)
    out, n, idx, nidx, info = C.POINTER(C.c_uint8)(), C.c_size_t(7), C.POINTER(C.c_uint8)(), C.c_size_t(7), ia.api.MpcDeltaInfo(-1, -1, -1)
    good = dict(d=enc.h, rgb=a.ctypes.data, stride=0, flags=0, interval=-1, out=C.byref(out), n=C.byref(n), idx=C.byref(idx), nidx=C.byref(nidx),
                info=C.byref(info))

    def call(**bad):
        v = dict(good, **bad)
        return L.mpc_delta_encode(v["d"], v["rgb"], v["stride"], None, v["flags"], v["interval"], v["out"], v["n"], v["idx"], v["nidx"], v["info"])

    for bad in (dict(d=None), dict(rgb=None), dict(out=None), dict(n=None), dict(info=None), dict(stride=3 * w - 1), dict(stride=1), dict(flags=8),
                dict(interval=0, idx=None), dict(interval=0, nidx=None), dict(interval=31), dict(interval=65537)):
        assert call(**bad) == ia.api.MPC_ERR_ARGUMENT, bad
    assert (n.value, nidx.value, info.key) == (7, 7, -1) and not out
    # a busy container job slot
    tiles = _all(name)
    d_counts, d_choices = torch.zeros(3 * tiles, dtype=torch.int16, device="cuda"), torch.zeros(3 * tiles * K, dtype=torch.int32, device="cuda")
    ctx.container_job_begin(1, d_counts.data_ptr(), d_choices.data_ptr(), w, h)
    assert call() == ia.api.MPC_ERR_ARGUMENT and b"slot 1" in L.mpc_last_error()
    ctx.container_job_cancel(1)
    # the session is as it was: the next call is a delta, and changed() is still the last successful call's
    assert enc.changed().size == tiles
    _step(enc, ctx, name, dc.bump(a, 10, 10), [1 * 6 + 1])
    assert call(stride=3 * w) == ia.api.MPC_OK and info.key == 0 and info.changed == 1   # back to `a`, the tight stride spelled out
    L.mpc_free(C.cast(out, C.c_void_p))
    # mpc_delta_changed: the count alone, a buffer too small, a null list
    got, cnt = np.zeros(4, np.int32), C.c_int(-1)
    p = got.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.mpc_delta_changed(enc.h, None, 0, C.byref(cnt)) == ia.api.MPC_OK and cnt.value == 1
    assert L.mpc_delta_changed(enc.h, p, 4, C.byref(cnt)) == ia.api.MPC_OK and got[0] == 7
    assert L.mpc_delta_changed(enc.h, None, 4, C.byref(cnt)) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_delta_changed(enc.h, p, 4, None) == ia.api.MPC_ERR_ARGUMENT
    _step(enc, ctx, name, a, None, is_key=1, key=True)
    assert L.mpc_delta_changed(enc.h, p, 4, C.byref(cnt)) == ia.api.MPC_ERR_ARGUMENT and cnt.value == tiles
    enc.close()


@pytest.mark.parametrize("name", ["ragged", "many"])
def test_host_frames_and_device_frames(ia, ctxs, name):
    """the same frames as host arrays of every stride and as device memory of every stride, a window at byte offset 1 of a larger buffer
    among them; a change in the surrounding buffer alone changes nothing"""
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    frames = dc.sequence(name, 4)
    host, dev = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
    for i, px in enumerate(frames):
        want_changed = dc.changed_tiles(frames[i - 1], px) if i else None
        kind = dc.STRIDES[i % 3]
        got = _step(host, ctx, name, dc.Layout(px, kind, 0, 70 + i).pixels, want_changed, is_key=int(i == 0))
        lay = dc.Layout(px, dc.STRIDES[(i + 1) % 3], i % 2, 80 + i)
        d_raw = _dev(lay.raw)
        assert dev.encode_device(d_raw.data_ptr() + lay.off, lay.stride, quant=dc.quant(name)) == got, (name, i)
        assert dev.info == host.info and (dev.changed() == host.changed()).all()
        assert (d_raw.cpu().numpy() == lay.raw).all()
    # the surrounding buffer alone changes, at byte offset 1 and with the tight stride spelled as 0
    px = frames[-1]
    for kind in dc.STRIDES:
        for seed in (1, 2):
            lay = dc.Layout(px, kind, 1, seed)
            d_raw = _dev(lay.raw)
            assert dev.encode_device(d_raw.data_ptr() + 1, lay.stride if kind != "tight" else 0) == _want(ctx, name, px)
            assert dev.info == (_all(name), 0, 0), (kind, seed, dev.info)
    host.close()
    dev.close()
