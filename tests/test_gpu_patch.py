"""The delta stream on the GPU (run with -m gpu): the unpack kernel alone against the model of tests/patch_cases.py, the sender
(every patch byte for byte the model's list and encode_image of the packed frame), the receiver (after every apply the kept frame is
the decode of that frame's whole container), refusals that leave the receiver exactly as it was, and host pixels against device pixels.
Every equality is exact.

The shapes are delta_cases.SHAPES, the smallest at which these kernels can go wrong: 83x45 is 11 x 6 tiles, ragged both ways, and
3 * 83 = 249 is no multiple of 8 -- its last tile column has 9 bytes, one whole chunk and one of a single byte; 5x3 and 8x8 are one
tile; 16x16 at K = 32 has full-length records; 200x136 is 425 tiles: a list of 424 packs seven columns with the last one partial, a
list of 65 opens a second column with one tile in it."""
import numpy as np
import pytest

import delta_cases as dc
import patch_cases as pc

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


_WANT, _DECODED, _PACKED = {}, {}, {}


def _want(ctx, name, px):
    """encode_image of a frame (a whole one or a packed one) with the shape's table: computed once per (table, flavour, pixels), shared"""
    q = dc.quant(name)
    key = (ctx.K, ctx.fast, None if q is None else np.asarray(q).tobytes(), np.asarray(px).shape, np.asarray(px).tobytes())
    if key not in _WANT:
        _WANT[key] = ctx.encode_image(np.ascontiguousarray(px), quant=q)
    return _WANT[key]


def _decoded(ctx, name, px):
    """what any decoder shows for the frame: decode_images of its whole container, once per frame and flavour"""
    blob = _want(ctx, name, px)
    key = (ctx.fast, blob)
    if key not in _DECODED:
        _DECODED[key] = np.array(ctx.decode_images([blob])[0])
    return _DECODED[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cases' own arrays stay as they are


def _ctx(ctxs, name):
    return ctxs[dc.SHAPES[name][2]]


def _all(name):
    w, h, _ = dc.SHAPES[name]
    return pc.tile_count(w, h)


def _stream(ctx, name):
    """[(frame, list or None, patch)]: patch_cases.stream with this context's encode_image"""
    return pc.stream(name, lambda px: _want(ctx, name, px))


# ---- the unpack kernel alone ----
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_unpack_kernel(ia, ctxs, name):
    import torch
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    paths = {True: 0, False: 0}
    for c, (label, lay, new, listed, rows) in enumerate(pc.unpack_cases(name)):
        n = len(listed)
        R, Cc, stride, _ = dc.pack_geometry(n, rows)
        key = (name, tuple(listed), rows)
        if key not in _PACKED:
            _PACKED[key] = dc.pack(new, listed, rows).reshape(8 * R, stride)
        d_list = _dev(np.asarray(listed, np.int32))
        for pad in (0, 16):                                                        # the packed stride tight and padded
            packed = torch.full((8 * R, stride + pad), 0xA5, dtype=torch.uint8, device="cuda")
            packed[:, :stride] = _dev(_PACKED[key])
            before = packed.cpu().numpy()
            dst = _dev(lay.raw)
            assert dst.data_ptr() % 8 == 0 and packed.data_ptr() % 8 == 0
            paths[(dst.data_ptr() + lay.off) % 8 == 0 and lay.stride % 8 == 0] += 1
            ctx.unpack_tiles_device(packed.data_ptr(), stride + pad if pad else 0, d_list.data_ptr(), n, rows, dst.data_ptr() + lay.off, w, h,
                                    lay.stride)
            torch.cuda.synchronize()
            want, bad = pc.unpack_raw(_PACKED[key], listed, lay.raw, lay.off, lay.stride, w, h, rows)
            got = dst.cpu().numpy()
            assert not bad and got.size == want.size
            assert (got == want).all(), (name, label, pad, np.flatnonzero(got != want)[:8])     # the whole buffer: guards, gaps, the room behind
            assert (packed.cpu().numpy() == before).all()
    assert paths[True] > 0 and paths[False] > 0                                    # the 8-byte stores and the byte stores
    # row_stride 0 is the tight stride
    old, new = dc.frame(w, h, 11), dc.frame(w, h, 12)
    dst, listed = _dev(old), [tiles - 1]
    packed, d_list = _dev(dc.pack(new, listed)), _dev(np.asarray(listed, np.int32))
    ctx.unpack_tiles_device(packed.data_ptr(), 0, d_list.data_ptr(), 1, 64, dst.data_ptr(), w, h, 0)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == pc.unpack(dc.pack(new, listed), listed, old)).all()
    # entries outside the frame write nothing and set the error word, which crop_records_check reads and clears
    lay = dc.Layout(old, "odd", pc.GUARD + 1, 9)
    listed = [0, tiles, -1, tiles - 1]
    packed_px = dc.pack(new, listed, 3)
    dst, packed, d_list = _dev(lay.raw), _dev(packed_px), _dev(np.asarray(listed, np.int32))
    with pytest.raises(ia.MpcError) as e:
        ctx.unpack_tiles_device(packed.data_ptr(), 0, d_list.data_ptr(), 4, 3, dst.data_ptr() + lay.off, w, h, lay.stride)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM
    assert ctx.L.mpc_crop_records_check(ctx.h, None) == ia.api.MPC_OK              # read and cleared
    want, bad = pc.unpack_raw(packed_px, listed, lay.raw, lay.off, lay.stride, w, h, 3)
    assert bad and (dst.cpu().numpy() == want).all()
    # refused with nothing enqueued
    for bad_args in (dict(packed_stride=28), dict(packed=packed.data_ptr() + 4), dict(n=0), dict(rows=0), dict(row_stride=3 * w - 1), dict(w=0)):
        v = dict(dict(packed=packed.data_ptr(), packed_stride=0, n=4, rows=3, w=w, row_stride=lay.stride), **bad_args)
        with pytest.raises(ia.MpcError) as e:
            ctx.unpack_tiles_device(v["packed"], v["packed_stride"], d_list.data_ptr(), v["n"], v["rows"], dst.data_ptr() + lay.off, v["w"], h,
                                    v["row_stride"])
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, bad_args
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == want).all()


# ---- the sender ----
def _send(enc, ctx, name, px, listed, patch, tiles, **kw):
    """one encode_patch: the bytes, the info and the list are the model's; listed None = a key patch"""
    got = enc.encode_patch(px, quant=dc.quant(name), **kw)
    assert got == patch, (name, enc.info, ctx.L.mpc_last_error())
    want = np.arange(tiles) if listed is None else np.asarray(listed, np.int32)
    assert enc.info == (tiles, want.size, int(listed is None)), (name, enc.info)
    assert (enc.changed() == want).all() and enc.changed().size == want.size
    return got


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_sender(ia, ctxs, name):
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    enc = ctx.delta_encoder(w, h)
    expected = _stream(ctx, name)
    for i, (px, listed, patch) in enumerate(expected):
        _send(enc, ctx, name, px, listed, patch, tiles)
        info = ia.patch_info(patch)
        assert (info["sequence"], info["key"], info["n"]) == (i, int(listed is None), tiles if listed is None else len(listed))
        if listed is None:                                                         # a key patch carries the whole frame's container
            assert patch == ia.patch_make(w, h, i, None, _want(ctx, name, px), key=True)
        elif listed:
            assert patch == ia.patch_make(w, h, i, listed, _want(ctx, name, dc.pack(px, listed)))
    seq = len(expected)
    # a frame equal to its predecessor: the 40-byte empty patch, and no pursuit launched
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    last = expected[-1][0]
    got = _send(enc, ctx, name, last, [], pc.make(w, h, seq, [], b""), tiles)
    assert len(got) == 40 and ctx.read_kernel_timing()[1] == 0
    ctx.kernel_timing(False)
    # a frame changed everywhere: a key patch, though the call is no key frame of the session
    other = np.array(dc.frame(w, h, 77))
    assert dc.changed_tiles(last, other).size == tiles
    _send(enc, ctx, name, other, None, ia.patch_make(w, h, seq + 1, None, _want(ctx, name, other), key=True), tiles)
    # MPC_DELTA_KEY on an unchanged frame: a key patch again; then nothing changed
    _send(enc, ctx, name, other, None, pc.make(w, h, seq + 2, None, _want(ctx, name, other), key=True), tiles, key=True)
    _send(enc, ctx, name, other, [], pc.make(w, h, seq + 3, [], b""), tiles)
    enc.close()


@pytest.mark.parametrize("name", ["ragged", "many"])
def test_encode_and_encode_patch_alternate(ia, ctxs, name):
    """one session, encode and encode_patch in turn: encode keeps its contract on every frame, the patches are numbered 1, 3, 5, ... and
    each is the patch against the frame before it, whichever call that frame went through"""
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    frames = dc.sequence(name) + [np.array(dc.frame(w, h, 78))]
    frames += [frames[-1], dc.change_tiles(frames[-1], [3, tiles - 1], 5)]
    enc = ctx.delta_encoder(w, h)
    for i, px in enumerate(frames):
        listed = [int(t) for t in dc.changed_tiles(frames[i - 1], px)] if i else None
        if i % 2 == 0:
            assert enc.encode(px, quant=dc.quant(name)) == _want(ctx, name, px), (name, i)
            assert enc.info == (tiles, tiles if i == 0 else len(listed), int(i == 0))
            assert (enc.changed() == (np.arange(tiles) if i == 0 else np.asarray(listed, np.int32))).all()
        elif len(listed) == tiles:
            _send(enc, ctx, name, px, None, pc.make(w, h, i, None, _want(ctx, name, px), key=True), tiles)
        else:
            container = _want(ctx, name, dc.pack(px, listed)) if listed else b""
            _send(enc, ctx, name, px, listed, pc.make(w, h, i, listed, container), tiles)
    enc.close()


@pytest.mark.parametrize("name", ["ragged", "many"])
def test_host_pixels_and_device_pixels(ia, ctxs, name):
    """the same frames as host arrays of every stride and as device memory of every stride, a window at byte offset 1 among them"""
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    host, dev = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
    for i, (px, listed, patch) in enumerate(_stream(ctx, name)):
        got = host.encode_patch(dc.Layout(px, dc.STRIDES[i % 3], 0, 70 + i).pixels, quant=dc.quant(name))
        lay = dc.Layout(px, dc.STRIDES[(i + 1) % 3], i % 2, 80 + i)
        d_raw = _dev(lay.raw)
        assert dev.encode_patch_device(d_raw.data_ptr() + lay.off, lay.stride, quant=dc.quant(name)) == got == patch, (name, i)
        assert dev.info == host.info and (dev.changed() == host.changed()).all()
        assert (d_raw.cpu().numpy() == lay.raw).all()
    host.close()
    dev.close()


# ---- the receiver ----
def _frame_device(ctx, dec, name):
    """the kept frame read through its device pointer: every tile of it packed by the pack kernel"""
    import torch
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    R, Cc, stride, _ = dc.pack_geometry(tiles)
    packed = torch.zeros((8 * R, stride), dtype=torch.uint8, device="cuda")
    d_list = _dev(np.arange(tiles, dtype=np.int32))
    ctx.pack_tiles_device(dec.frame_device(), w, h, 0, d_list.data_ptr(), tiles, dc.PACK_ROWS, packed.data_ptr())
    torch.cuda.synchronize()
    return packed.cpu().numpy().reshape(8 * R, 8 * Cc, 3)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_receiver(ia, ctxs, name, fast):
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    try:
        ctx.set_fast(fast)
        expected = _stream(ctx, name)                                              # host-made: patch_cases.make of this flavour's containers
        enc = ctx.delta_encoder(w, h)
        sent = [enc.encode_patch(px, quant=dc.quant(name)) for px, _, _ in expected]
        enc.close()
        for source, patches in (("host", [patch for _, _, patch in expected]), ("sender", sent)):
            dec = ctx.patch_decoder(w, h)
            assert (dec.frame() == 0).all() and dec.changed().size == 0            # black until the first key patch
            for i, ((px, listed, _), patch) in enumerate(zip(expected, patches)):
                info = dec.apply(patch)
                assert info == ia.patch_info(patch) and info["sequence"] == i
                assert (dec.frame() == _decoded(ctx, name, px)).all(), (name, fast, source, i)
                want = np.arange(tiles) if listed is None else np.asarray(listed, np.int32)
                assert (dec.changed() == want).all() and dec.changed().size == want.size
                assert (_frame_device(ctx, dec, name) == dc.pack(dec.frame(), list(range(tiles)))).all()
            dec.close()
    finally:
        ctx.set_fast(False)


def _state(ia, dec):
    """(frame, list, expected sequence or None before a key patch): the last from the text of a refusal that changes nothing, a patch
    whose sequence number is never due"""
    w, h = dec.width, dec.height
    with pytest.raises(ia.MpcError) as e:
        dec.apply(pc.make(w, h, 2**32 - 1, [], b""))
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "4294967295" in str(e.value)
    words = str(e.value).split()
    due = int(words[words.index("where") + 2]) if "where" in words else None
    return dec.frame(), dec.changed().copy(), due


def _refused(ia, dec, patch, status, label):
    frame, listed, due = _state(ia, dec)
    with pytest.raises(ia.MpcError) as e:
        dec.apply(patch)
    assert e.value.status == status, (label, str(e.value))
    after = _state(ia, dec)
    assert (after[0] == frame).all() and after[1].tolist() == listed.tolist() and after[2] == due, label
    return str(e.value)


def _payload_flip(ia, container):
    """the container with one payload bit flipped so that read_compressed refuses it while its header still reads the same: the first
    such bit from the container's end, found on the host"""
    size = ia.container_info(container)
    for bit in range(8 * len(container) - 1, 8 * 24, -1):
        flipped = bytearray(container)
        flipped[bit // 8] ^= 1 << (bit % 8)
        flipped = bytes(flipped)
        try:
            ia.read_compressed(flipped)
        except ia.MpcError:
            if ia.container_info(flipped) == size:
                return flipped
    raise AssertionError("no refused flip found")


def test_refusals_are_atomic(ia, ctxs):
    name = "ragged"
    ctx, ctx32 = ctxs[8], ctxs[32]
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    A, S = ia.api.MPC_ERR_ARGUMENT, ia.api.MPC_ERR_BITSTREAM
    expected = _stream(ctx, name)
    patches = [patch for _, _, patch in expected]
    kinds = [None if listed is None else len(listed) for _, listed, _ in expected]
    t = next(i for i, k in enumerate(kinds) if k)                                  # the first tile patch
    assert kinds[0] is None and t >= 1
    dec = ctx.patch_decoder(w, h)
    # a non-key patch on a fresh session, and the sequence number does not matter
    text = _refused(ia, dec, patches[t], A, "no key yet")
    assert str(t) in text
    _refused(ia, dec, pc.make(w, h, 0, [], b""), A, "no key yet, empty")
    for i in range(t):
        dec.apply(patches[i])
    # skipped and repeated
    text = _refused(ia, dec, patches[t + 1], A, "skipped") if ia.patch_info(patches[t + 1])["key"] == 0 else ""
    assert not text or (str(t + 1) in text and str(t) in text)                     # both numbers
    dec.apply(patches[t])
    assert (dec.frame() == _decoded(ctx, name, expected[t][0])).all()
    text = _refused(ia, dec, patches[t], A, "repeated")
    assert f"patch {t} where patch {t + 1}" in text
    # the session's geometry off by one tile, either way
    for dw, dh in ((8, 0), (0, 8), (-8, 0)):
        off = ctx.patch_decoder(w + dw, h + dh)
        _refused(ia, off, patches[0], A, "geometry")
        off.close()
    # a patch of a K = 8 context on a K = 32 one
    dec32 = ctx32.patch_decoder(w, h)
    _refused(ia, dec32, patches[0], A, "K")
    dec32.close()
    # the next patch, damaged: a container the decoder refuses, one of another packed size, and every hostile blob
    nxt = next(i for i in range(t + 1, len(kinds)) if kinds[i])                     # the next tile patch ...
    for i in range(t + 1, nxt):
        dec.apply(patches[i])                                                      # ... with whatever lies in between applied
    px, listed, patch = expected[nxt]
    info = ia.patch_info(patch)
    container = patch[info["container_offset"]:]
    _refused(ia, dec, ia.patch_make(w, h, nxt, listed, _payload_flip(ia, container)), S, "a refused container")
    more = sorted(listed + [min(set(range(tiles)) - set(listed))])                # one tile more: another packed frame
    assert len(more) == len(listed) + 1 and dc.pack_geometry(len(more))[:2] != dc.pack_geometry(len(listed))[:2]
    _refused(ia, dec, pc.make(w, h, nxt, listed, _want(ctx, name, dc.pack(px, more))), S, "another packed size")
    _refused(ia, dec, pc.make(w, h, nxt, None, _want(ctx, name, dc.pack(px, more)), key=True), S, "a key patch's container of another size")
    key, empty = pc.make(w, h, nxt, None, _want(ctx, name, px), key=True), pc.make(w, h, nxt, [], b"")
    frame, kept_list, due = _state(ia, dec)
    for label, blob in pc.hostile(patch, key, empty, _want(ctx, name, dc.pack(px, more))):
        with pytest.raises(ia.MpcError) as e:
            dec.apply(blob)
        assert e.value.status == S, label
    after = _state(ia, dec)
    assert (after[0] == frame).all() and after[1].tolist() == kept_list.tolist() and after[2] == due == nxt
    # and the next valid patches still apply and give the right frames
    for i in range(nxt, len(patches)):
        dec.apply(patches[i])
        assert (dec.frame() == _decoded(ctx, name, expected[i][0])).all(), i
        assert dec.changed().tolist() == (list(range(tiles)) if expected[i][1] is None else expected[i][1])
    # a key patch resynchronises at any sequence number
    dec.apply(pc.make(w, h, 1000, None, _want(ctx, name, expected[0][0]), key=True))
    assert (dec.frame() == _decoded(ctx, name, expected[0][0])).all() and _state(ia, dec)[2] == 1001
    dec.close()
