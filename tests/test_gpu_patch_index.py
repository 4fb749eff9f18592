"""Patches that carry their container's seek index, on the GPU (run with -m gpu): the sender (mpc_delta_encode_patch_indexed gives byte
for byte mpc_patch_add_index of what mpc_delta_encode_patch gives, in any mix of the session's calls, for host and device pixels), the
receiver (a version-2 patch decodes through the indexed route to exactly the frame its version-1 twin gives, and says so:
last_route), the index as a hint (a damaged index section costs the route, never the frame) and the refusals (status, text and
atomicity are those of the stripped patch).  Every equality is exact.

The shapes are delta_cases.SHAPES, the frames patch_index_cases.frames: patch_cases's stream and behind it lists of 424 of 425 tiles,
65 tiles and a third of the tiles.  The intervals are 32, the smallest, and the default.  Before a device route is asserted the same
container and index go through the host's chunked parse (mpc_parse_container_by_index), which must report route 0: the device's
answer is then no silently refused index."""
import numpy as np
import pytest

import delta_cases as dc
import patch_cases as pc
import patch_index_cases as pic

pytestmark = pytest.mark.gpu

BIG = 2**40                                     # an index_min_bytes above every container


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


_WANT, _DECODED, _ROUTE0 = {}, {}, set()


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
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _ctx(ctxs, name):
    return ctxs[dc.SHAPES[name][2]]


def _all(name):
    w, h, _ = dc.SHAPES[name]
    return pc.tile_count(w, h)


def _stream(ctx, name):
    """[(frame, list or None, version-1 patch)]: patch_index_cases.stream with this context's encode_image"""
    return pic.stream(name, lambda px: _want(ctx, name, px))


def _indexed(ia, patch, interval):
    """patch_add_index of a patch, and -- the precondition of every route-0 assertion -- its container and index section through the
    host's chunked parse, which must accept the index"""
    out = ia.patch_add_index(patch, interval)
    at, size = ia.patch_index(out)
    if size and out not in _ROUTE0:
        info = ia.patch_info(out)
        container = out[info["container_offset"]:at]
        assert ia.parse_container_by_index(container, out[at:])[1] == 0
        _ROUTE0.add(out)
    return out


# ---- the sender ----
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_sender(ia, ctxs, name):
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    expected = _stream(ctx, name)
    twin = ctx.delta_encoder(w, h)
    plain = []
    for px, listed, patch in expected:
        plain.append(twin.encode_patch(px, quant=dc.quant(name)))
        assert plain[-1] == patch
    twin.close()
    versions = set()
    for interval, least in ((32, 0), (0, 0), (32, BIG), (0, BIG), (-1, 0)):
        enc = ctx.delta_encoder(w, h)
        for i, ((px, listed, _), P) in enumerate(zip(expected, plain)):
            got = enc.encode_patch(px, quant=dc.quant(name), index_interval=interval, index_min_bytes=least)
            assert got == (P if interval < 0 else ia.patch_add_index(P, interval, least)), (name, interval, least, i, ctx.L.mpc_last_error())
            n = tiles if listed is None else len(listed)
            assert (ia.patch_index(got)[1] > 0) == (interval >= 0 and least == 0 and n > 0)
            assert ia.patch_strip_index(got) == P and ia.patch_info(got) == ia.patch_info(P)
            assert enc.info == (tiles, n, int(listed is None)), (name, enc.info)
            want = np.arange(tiles) if listed is None else np.asarray(listed, np.int32)
            assert (enc.changed() == want).all() and enc.changed().size == want.size
            versions.add((interval, least, got[4]))
            if interval >= 0 and least == 0 and n > 0:
                assert got == _indexed(ia, P, interval)                            # and the host's parse accepts what the sender attached
        enc.close()
    assert {(32, 0, 2), (0, 0, 2)} <= versions and not {v for v in versions if v[2] == 2 and (v[1] or v[0] < 0)}
    # the boundary of index_min_bytes on a real patch, and mpc_delta_encode's interval refusals, which leave the session as it was
    enc = ctx.delta_encoder(w, h)
    px, _, P = expected[0]
    cb = ia.patch_info(P)["container_bytes"]
    assert enc.encode_patch(px, quant=dc.quant(name), key=True, index_interval=32, index_min_bytes=cb)[4] == 2
    assert enc.encode_patch(px, quant=dc.quant(name), key=True, index_interval=32, index_min_bytes=cb + 1)[4] == 1
    for bad in (1, 31, 65537):
        with pytest.raises(ia.MpcError) as e:
            enc.encode_patch(px, quant=dc.quant(name), index_interval=bad)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    got = enc.encode_patch(px, quant=dc.quant(name), index_interval=32, index_min_bytes=0)
    assert got == pc.make(w, h, 2, [], b"") and enc.info == (tiles, 0, 0)              # still the session's third call, nothing changed
    enc.close()


@pytest.mark.parametrize("name", ["ragged", "many"])
def test_the_three_encode_calls_alternate(ia, ctxs, name):
    """one session calls encode, encode_patch and the indexed encode_patch in turn; its twin calls encode_patch alone: the lists are
    identical, and every patch, stripped, is the twin's"""
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    frames = pic.frames(name)
    for start in range(3):
        enc, twin = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
        for i, px in enumerate(frames):
            P = twin.encode_patch(px, quant=dc.quant(name))
            kind = (i + start) % 3
            if kind == 0:
                blob, index = enc.encode(px, quant=dc.quant(name), index_interval=32)
                assert blob == _want(ctx, name, px) and index == ia.container_index(blob, 32, expanded=True), (name, start, i)
            elif kind == 1:
                assert enc.encode_patch(px, quant=dc.quant(name)) == P, (name, start, i)
            else:
                got = enc.encode_patch(px, quant=dc.quant(name), index_interval=32 if i % 2 else 0, index_min_bytes=0)
                assert got == ia.patch_add_index(P, 32 if i % 2 else 0) and ia.patch_strip_index(got) == P, (name, start, i)
            assert (enc.changed() == twin.changed()).all() and enc.changed().size == twin.changed().size
            assert enc.info[:2] == twin.info[:2]                                   # key: encode reports the call, a patch call the patch
            assert ia.patch_info(P)["sequence"] == i
        enc.close()
        twin.close()


@pytest.mark.parametrize("name", ["ragged", "many"])
def test_host_pixels_and_device_pixels(ia, ctxs, name):
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    host, dev = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
    for i, (px, listed, patch) in enumerate(_stream(ctx, name)):
        interval = 32 if i % 2 else 0
        got = host.encode_patch(dc.Layout(px, dc.STRIDES[i % 3], 0, 70 + i).pixels, quant=dc.quant(name), index_interval=interval, index_min_bytes=0)
        lay = dc.Layout(px, dc.STRIDES[(i + 1) % 3], i % 2, 80 + i)
        d_raw = _dev(lay.raw)
        sent = dev.encode_patch_device(d_raw.data_ptr() + lay.off, lay.stride, quant=dc.quant(name), index_interval=interval, index_min_bytes=0)
        assert sent == got == ia.patch_add_index(patch, interval), (name, i)
        assert dev.info == host.info and (dev.changed() == host.changed()).all()
        assert (d_raw.cpu().numpy() == lay.raw).all()
    host.close()
    dev.close()


# ---- the receiver ----
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_receiver_both_flavours_of_patch(ia, ctxs, name, fast):
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    try:
        ctx.set_fast(fast)
        expected = _stream(ctx, name)
        for interval in pic.INTERVALS:
            one, two, mixed = ctx.patch_decoder(w, h), ctx.patch_decoder(w, h), ctx.patch_decoder(w, h)
            assert one.last_route() == two.last_route() == -1                      # no apply yet
            seen = set()
            for i, (px, listed, patch) in enumerate(expected):
                indexed = _indexed(ia, patch, interval)
                n = tiles if listed is None else len(listed)
                assert (indexed[4], ia.patch_index(indexed)[1] > 0) == ((2, True) if n else (1, False))
                info1, info2, info3 = one.apply(patch), two.apply(indexed), mixed.apply(indexed if i % 2 else patch)
                assert info1 == info2 == info3 == ia.patch_info(patch) and info1["sequence"] == i
                frame = two.frame()
                assert (frame == one.frame()).all() and (frame == mixed.frame()).all(), (name, fast, interval, i)
                assert (frame == _decoded(ctx, name, px)).all(), (name, fast, interval, i)
                want = np.arange(tiles) if listed is None else np.asarray(listed, np.int32)
                for dec in (one, two, mixed):
                    assert (dec.changed() == want).all() and dec.changed().size == want.size
                assert one.last_route() == (1 if n else -1), (name, i)
                assert two.last_route() == (0 if n else -1), (name, fast, interval, i, n)
                assert mixed.last_route() == (-1 if not n else 0 if i % 2 else 1)
                seen.add("key" if listed is None else "tile" if n else "empty")
            assert seen == ({"key", "tile", "empty"} if tiles > 1 else {"key", "empty"})
            for dec in (one, two, mixed):
                dec.close()
    finally:
        ctx.set_fast(False)


def _key_before(ctx, name, expected, t):
    """a key patch that leaves a receiver where patch t is due: frame t - 1's whole container under sequence t - 1"""
    w, h, _ = dc.SHAPES[name]
    return pc.make(w, h, t - 1, None, _want(ctx, name, expected[t - 1][0]), key=True)


@pytest.mark.parametrize("name", ["ragged", "many", "full"])
def test_the_index_is_only_a_hint(ia, ctxs, name):
    ctx = _ctx(ctxs, name)
    w, h, _ = dc.SHAPES[name]
    expected = _stream(ctx, name)
    t = max((i for i, (_, listed, _) in enumerate(expected) if listed), key=lambda i: len(expected[i][1]))      # the longest tile patch
    key2, tile2 = _indexed(ia, expected[0][2], 32), _indexed(ia, expected[t][2], 32)
    key_index, tile_index = key2[ia.patch_index(key2)[0]:], tile2[ia.patch_index(tile2)[0]:]
    dec = ctx.patch_decoder(w, h)
    routes = set()
    for label, blob, serial in pic.damaged(key2, tile_index, 1):
        assert ia.patch_info(blob) == ia.patch_info(key2) and ia.patch_strip_index(blob) == expected[0][2]      # a valid patch
        dec.apply(_key_before(ctx, name, expected, t))                             # another frame first
        dec.apply(blob)
        assert (dec.frame() == _decoded(ctx, name, expected[0][0])).all(), (name, "key", label)
        assert dec.last_route() in ((1,) if serial else (0, 1)), (name, "key", label, dec.last_route())
        routes.add(dec.last_route())
    for label, blob, serial in pic.damaged(tile2, key_index, 2):
        assert ia.patch_info(blob) == ia.patch_info(tile2) and ia.patch_strip_index(blob) == expected[t][2]
        dec.apply(_key_before(ctx, name, expected, t))
        dec.apply(blob)
        assert (dec.frame() == _decoded(ctx, name, expected[t][0])).all(), (name, "tile", label)
        assert dec.changed().tolist() == expected[t][1]
        assert dec.last_route() in ((1,) if serial else (0, 1)), (name, "tile", label, dec.last_route())
        routes.add(dec.last_route())
    assert 1 in routes
    # and the undamaged ones, from the same state: parsed on the device
    dec.apply(_key_before(ctx, name, expected, t))
    dec.apply(tile2)
    assert dec.last_route() == 0 and (dec.frame() == _decoded(ctx, name, expected[t][0])).all()
    dec.apply(key2)
    assert dec.last_route() == 0 and (dec.frame() == _decoded(ctx, name, expected[0][0])).all()
    dec.close()


# ---- refusals ----
def _state(ia, dec):
    """(frame, list, expected sequence or None before a key patch, last_route): the third from the text of a refusal that changes nothing,
    a patch whose sequence number is never due"""
    w, h = dec.width, dec.height
    with pytest.raises(ia.MpcError) as e:
        dec.apply(pc.make(w, h, 2**32 - 1, [], b""))
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "4294967295" in str(e.value)
    words = str(e.value).split()
    due = int(words[words.index("where") + 2]) if "where" in words else None
    return dec.frame(), dec.changed().copy(), due, dec.last_route()


def _same(a, b):
    return (a[0] == b[0]).all() and a[1].tolist() == b[1].tolist() and a[2:] == b[2:]


def _refused(ia, dec, twin, patch, status, label):
    """`patch` (version 2) is refused by `dec` exactly as its stripped twin is by `twin`, a session in the same state fed version-1 patches;
    both are left as they were"""
    before, twin_before = _state(ia, dec), _state(ia, twin)
    with pytest.raises(ia.MpcError) as e:
        dec.apply(patch)
    with pytest.raises(ia.MpcError) as e1:
        twin.apply(pic.cut(patch))
    assert e.value.status == e1.value.status == status, (label, str(e.value), str(e1.value))
    assert str(e.value) == str(e1.value), label
    assert _same(_state(ia, dec), before) and _same(_state(ia, twin), twin_before), label
    return str(e.value)


def _payload_flip(ia, container):
    """the container with one payload bit flipped so that read_compressed refuses it while its header still reads the same: the first
    such bit from the container's end, found on the host (test_gpu_patch.py's damage)"""
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


def test_refusals_are_atomic_and_unchanged(ia, ctxs):
    name = "ragged"
    ctx, ctx32 = ctxs[8], ctxs[32]
    w, h, _ = dc.SHAPES[name]
    tiles = _all(name)
    A, S = ia.api.MPC_ERR_ARGUMENT, ia.api.MPC_ERR_BITSTREAM
    expected = _stream(ctx, name)
    plain = [patch for _, _, patch in expected]
    patches = [_indexed(ia, patch, 32) for patch in plain]
    kinds = [None if listed is None else len(listed) for _, listed, _ in expected]
    t = next(i for i, k in enumerate(kinds) if k)                                  # the first tile patch
    assert kinds[0] is None and t >= 1 and patches[t][4] == 2 and patches[0][4] == 2
    dec, twin = ctx.patch_decoder(w, h), ctx.patch_decoder(w, h)
    # a non-key patch before any key patch
    text = _refused(ia, dec, twin, patches[t], A, "no key yet")
    assert str(t) in text and dec.last_route() == -1
    for i in range(t):
        dec.apply(patches[i])
        twin.apply(plain[i])
    # a wrong sequence: skipped, repeated
    if ia.patch_info(patches[t + 1])["key"] == 0 and kinds[t + 1]:
        text = _refused(ia, dec, twin, patches[t + 1], A, "skipped")
        assert str(t + 1) in text and str(t) in text
    dec.apply(patches[t])
    twin.apply(plain[t])
    assert dec.last_route() == 0 and twin.last_route() == 1
    assert (dec.frame() == _decoded(ctx, name, expected[t][0])).all()
    text = _refused(ia, dec, twin, patches[t], A, "repeated")
    assert f"patch {t} where patch {t + 1}" in text
    # a wrong size, either way; a wrong K
    for dw, dh in ((8, 0), (0, 8), (-8, 0)):
        off, off1 = ctx.patch_decoder(w + dw, h + dh), ctx.patch_decoder(w + dw, h + dh)
        _refused(ia, off, off1, patches[0], A, "geometry")
        off.close()
        off1.close()
    dec32, twin32 = ctx32.patch_decoder(w, h), ctx32.patch_decoder(w, h)
    _refused(ia, dec32, twin32, patches[0], A, "K")
    dec32.close()
    twin32.close()
    # the next tile patch with its container's payload damaged: the decoder's own refusal, whichever route met it.  The index section is
    # the undamaged container's, then one cut to its header, then none that the format would allow
    nxt = next(i for i in range(t + 1, len(kinds)) if kinds[i])
    for i in range(t + 1, nxt):
        dec.apply(patches[i])
        twin.apply(plain[i])
    px, listed, patch = expected[nxt]
    info = ia.patch_info(patch)
    container = patch[info["container_offset"]:]
    flipped = _payload_flip(ia, container)
    index = ia.container_index(container, 32)
    _refused(ia, dec, twin, pic.make(w, h, nxt, listed, flipped, index=index), S, "a refused container, its old index")
    _refused(ia, dec, twin, pic.make(w, h, nxt, listed, flipped, index=index[:56]), S, "a refused container, an index that is none")
    whole = _want(ctx, name, px)
    _refused(ia, dec, twin, pic.make(w, h, nxt, None, _payload_flip(ia, whole), key=True, index=ia.container_index(whole, 32)), S,
             "a refused key container")
    # a container of another packed size under a valid index of its own
    more = sorted(listed + [min(set(range(tiles)) - set(listed))])
    assert dc.pack_geometry(len(more))[:2] != dc.pack_geometry(len(listed))[:2]
    other = _want(ctx, name, dc.pack(px, more))
    _refused(ia, dec, twin, pic.make(w, h, nxt, listed, other, index=ia.container_index(other, 32)), S, "another packed size")
    # the hostile version-2 corpus
    before = _state(ia, dec)
    for label, blob in pic.hostile(patches[nxt], _indexed(ia, pc.make(w, h, nxt, None, whole, key=True), 32), pc.make(w, h, nxt, [], b"")):
        with pytest.raises(ia.MpcError) as e:
            dec.apply(blob)
        assert e.value.status == S, label
    after = _state(ia, dec)
    assert _same(after, before) and after[2] == nxt and after[3] == (0 if kinds[nxt - 1] != 0 else -1)
    # and the next good patches are accepted
    for i in range(nxt, len(patches)):
        dec.apply(patches[i])
        assert (dec.frame() == _decoded(ctx, name, expected[i][0])).all(), i
        assert dec.changed().tolist() == (list(range(tiles)) if expected[i][1] is None else expected[i][1])
        assert dec.last_route() == (0 if kinds[i] != 0 else -1)
    dec.close()
    twin.close()
