"""The delta stream on the host: the patch format's writer and parser (mpc_patch_make, mpc_patch_info, mpc_patch_tiles) against the
pure-Python model of tests/patch_cases.py, the blobs every parser must refuse, the unpack model against delta_cases.pack and against
the mistakes its cases are there to catch, and a whole stream through the oracle.  No GPU.  Every equality is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import delta_cases as dc
import patch_cases as pc
from conftest import ROOT


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def blank_container(ia, w, h, K=8):
    """a valid container of w x h pixels made on the host: every tile-channel of length 0"""
    tiles = pc.tile_count(w, h)
    return ia.assemble_streams(w, h, K, 8, ia.quant_tables(K, dc.QUALITY), np.zeros((tiles, 3), np.uint16), np.zeros((tiles, 3, K), np.uint32))


def packed_container(ia, n):
    R, Cc, _, _ = dc.pack_geometry(n)
    return blank_container(ia, 8 * Cc, 8 * R)


def _agree(ia, w, h, sequence, tiles, container, key=False):
    """the library's writer gives the model's bytes, and both parsers read them alike"""
    want = pc.make(w, h, sequence, tiles, container, key)
    got = ia.patch_make(w, h, sequence, tiles, container, key)
    assert got == want, (w, h, sequence, key)
    model = pc.parse(got)
    listed = model.pop("list")
    assert ia.patch_info(got) == model
    assert ia.patch_tiles(got).tolist() == listed and ia.patch_tiles(got).dtype == np.int32
    return got


def test_the_writer_and_the_parsers_are_the_model(ia):
    # 16384 x 16384 is 2048 x 2048 tiles: room for a gap of 2 097 152
    w = h = 16384
    tiles = pc.tile_count(w, h)
    listed, t = [0], 0
    for gap in (0, 127, 128, 16383, 16384, 2097152):
        t += gap + 1
        listed.append(t)
    listed.append(tiles - 1)
    assert pc.gaps(listed)[:7] == [0, 0, 127, 128, 16383, 16384, 2097152] and [len(pc.leb128(g)) for g in pc.gaps(listed)[1:7]] == [1, 1, 2, 2, 3, 4]
    blob = _agree(ia, w, h, 7, listed, packed_container(ia, len(listed)))
    assert pc.parse(blob)["list"] == listed
    _agree(ia, w, h, 2**32 - 1, [tiles - 1], packed_container(ia, 1))                  # n = 1, the last tile, the largest sequence
    _agree(ia, w, h, 0, [0], packed_container(ia, 1))
    _agree(ia, w, h, 1, [2097152, tiles - 1], packed_container(ia, 2))         # the first gap of four bytes
    # n = tiles - 1, with and without tile 0; key; empty
    for name in ("ragged", "many", "full"):
        sw, sh, _ = dc.SHAPES[name]
        all_tiles = pc.tile_count(sw, sh)
        for skip in (0, all_tiles // 2, all_tiles - 1):
            listed = [t for t in range(all_tiles) if t != skip]
            _agree(ia, sw, sh, 3, listed, packed_container(ia, all_tiles - 1))
        key = _agree(ia, sw, sh, 4, None, blank_container(ia, sw, sh), key=True)
        assert ia.patch_info(key)["key"] == 1 and ia.patch_tiles(key).tolist() == list(range(all_tiles))
        empty = _agree(ia, sw, sh, 5, [], b"")
        assert len(empty) == 40 and ia.patch_info(empty)["n"] == 0 and ia.patch_tiles(empty).size == 0
    one = _agree(ia, 8, 8, 0, None, blank_container(ia, 8, 8), key=True)                # one tile: only key and empty exist
    assert ia.patch_info(one)["tiles"] == 1


def _valid(ia):
    w, h, _ = dc.SHAPES["ragged"]
    tile = ia.patch_make(w, h, 9, [5, 40], packed_container(ia, 2))
    key = ia.patch_make(w, h, 9, None, blank_container(ia, w, h), key=True)
    empty = ia.patch_make(w, h, 9, [], None)
    return tile, key, empty, blank_container(ia, 8, 24)


def test_hostile_blobs_are_refused(ia):
    L = ia.load_library()
    tile, key, empty, other = _valid(ia)
    for good in (tile, key, empty):
        ia.patch_info(good)
        pc.parse(good)
    cases = pc.hostile(tile, key, empty, other)
    labels = {label for label, _ in cases}
    assert {"wrong magic", "wrong version", "a reserved flag bit", "a nonzero reserved word", "list_bytes one too small", "list_bytes one too large",
            "a 6-byte varint", "a trailing 0x00 group", "a value of 2^31", "last tile = tiles", "n one too small", "n one too large",
            "a key patch with a list", "an empty patch with a container", "a tile patch without a container", "n == tiles without the key flag",
            "trailing bytes", "container_bytes beyond the blob", "a tile patch's container of another size"} <= labels
    assert sum(label.startswith("prefix ") for label in labels) == len(tile)
    info, n = ia.api.MpcPatchInfo(), C.c_int(-7)
    for label, blob in cases:
        with pytest.raises(pc.Refused):
            pc.parse(blob)
        # on an exact-size buffer of its own
        buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
        assert L.mpc_patch_info(buf, len(blob), C.byref(info)) == ia.api.MPC_ERR_BITSTREAM, label
        assert L.mpc_last_error()
        assert L.mpc_patch_tiles(buf, len(blob), None, 0, C.byref(n)) == ia.api.MPC_ERR_BITSTREAM, label
    assert n.value == -7                                             # a refusal writes nothing


def test_argument_refusals(ia):
    L = ia.load_library()
    tile, key, empty, other = _valid(ia)
    w, h, _ = dc.SHAPES["ragged"]
    cont = packed_container(ia, 2)
    for bad in (dict(tiles=[40, 5]), dict(tiles=[5, 5]), dict(tiles=[5, 66]), dict(tiles=[-1, 5]), dict(tiles=list(range(66))),
                dict(tiles=[5, 40], container=None), dict(tiles=[], container=cont), dict(w=0), dict(h=0), dict(w=2**31 - 1, h=2**31 - 1),
                dict(key=True, container=None)):
        v = dict(dict(w=w, h=h, tiles=[5, 40], container=cont, key=False), **bad)
        with pytest.raises(ia.MpcError) as e:
            ia.patch_make(v["w"], v["h"], 0, v["tiles"], v["container"], v["key"])
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, bad
    buf = (C.c_uint8 * len(tile)).from_buffer_copy(tile)
    info, n, out, nb = ia.api.MpcPatchInfo(), C.c_int(-7), C.POINTER(C.c_uint8)(), C.c_size_t(0)
    got = np.zeros(4, np.int32)
    p = got.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.mpc_patch_info(None, 40, C.byref(info)) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_info(buf, len(tile), None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_make(w, h, 0, 0, p, 0, None, 0, None, C.byref(nb)) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_make(w, h, 0, 0, p, 0, None, 0, C.byref(out), None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_make(w, h, 0, 0, None, 2, buf, 8, C.byref(out), C.byref(nb)) == ia.api.MPC_ERR_ARGUMENT and not out
    # mpc_patch_tiles follows mpc_delta_changed: the count alone, a buffer too small, a null list
    assert L.mpc_patch_tiles(buf, len(tile), None, 0, C.byref(n)) == ia.api.MPC_OK and n.value == 2
    assert L.mpc_patch_tiles(buf, len(tile), p, 4, C.byref(n)) == ia.api.MPC_OK and got.tolist() == [5, 40, 0, 0]
    assert L.mpc_patch_tiles(buf, len(tile), p, 1, C.byref(n)) == ia.api.MPC_ERR_ARGUMENT and n.value == 2 and got.tolist() == [5, 40, 0, 0]
    assert L.mpc_patch_tiles(buf, len(tile), None, 4, C.byref(n)) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_tiles(buf, len(tile), p, 4, None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_tiles(None, len(tile), p, 4, C.byref(n)) == ia.api.MPC_ERR_ARGUMENT
    # a host-only context: no receiver, no kernel
    ctx = ia.create_compression_context(4, 8, 3.5)
    with pytest.raises(ia.MpcError) as e:
        ctx.patch_decoder(16, 16)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    with pytest.raises(ia.MpcError) as e:
        ctx.unpack_tiles_device(8, 0, 8, 1, 64, 8, 8, 8)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    hnd = C.c_void_p()
    assert L.mpc_patch_decoder_create(ctx.h, 0, 8, C.byref(hnd)) == ia.api.MPC_ERR_ARGUMENT and not hnd
    assert L.mpc_patch_decoder_create(ctx.h, 8, 8, None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_patch_decoder_create(None, 8, 8, C.byref(hnd)) == ia.api.MPC_ERR_ARGUMENT
    L.mpc_patch_decoder_destroy(None)                                # a no-op
    ctx.close()


def test_the_declared_symbols_exist(ia):
    L = ia.load_library()
    text = open(os.path.join(ROOT, "include", "mpcodec.h")).read()
    section = text.split("patch: send only the changed tiles")[1].split("budget: encode to a byte budget")[0].split("*/", 1)[1]
    names = set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", section, flags=re.S)))
    want = {"mpc_patch_make", "mpc_patch_info", "mpc_patch_tiles", "mpc_delta_encode_patch", "mpc_unpack_tiles_device", "mpc_patch_decoder_create",
            "mpc_patch_decoder_destroy", "mpc_patch_apply", "mpc_patch_frame_device", "mpc_patch_read", "mpc_patch_changed"}
    assert names == want
    for name in want:
        assert hasattr(L, name), name


# ---- the unpack model ----
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_unpack_inverts_pack(name):
    w, h, _ = dc.SHAPES[name]
    old, new = dc.frame(w, h, 11), dc.frame(w, h, 12)
    tx, ty = dc.grid(w, h)
    for label, tiles in pc.tile_lists(name).items():
        got = pc.unpack(dc.pack(new, tiles), tiles, old)
        listed = np.zeros((tx, ty), bool)
        listed.reshape(-1)[tiles] = True
        mask = np.repeat(np.repeat(listed.T, 8, axis=0), 8, axis=1)[:h, :w]
        assert (got[mask] == new[mask]).all() and (got[~mask] == old[~mask]).all(), (name, label)
        assert (pc.unpack(dc.pack(got, tiles), tiles, got) == got).all()
        assert (dc.pack(got, tiles) == dc.pack(new, tiles)).all()
    # an unsorted list and other row counts are the pack's inverse too
    tiles = list(np.random.default_rng(5).permutation(tx * ty)[:max(tx * ty // 2, 1)])
    for rows in (1, 3, 64):
        got = pc.unpack(dc.pack(new, tiles, rows), tiles, old, rows)
        assert (dc.pack(got, tiles, rows) == dc.pack(new, tiles, rows)).all()
        assert (dc.changed_tiles(old, got) == dc.changed_tiles(old, pc.unpack(dc.pack(new, sorted(tiles)), sorted(tiles), old))).all()


def test_an_entry_outside_the_frame_writes_nothing():
    w, h, _ = dc.SHAPES["ragged"]
    old, new = dc.frame(w, h, 11), dc.frame(w, h, 12)
    lay = dc.Layout(old, "odd", pc.GUARD, 1)
    tiles = [0, 66, -1, 65]
    got, bad = pc.unpack_raw(dc.pack(new, tiles, 3), tiles, lay.raw, lay.off, lay.stride, w, h, 3)
    want, ok = pc.unpack_raw(dc.pack(new, [0, 65], 2), [0, 65], lay.raw, lay.off, lay.stride, w, h, 2)
    assert bad and not ok and (got == want).all() and (got != lay.raw).any()


@pytest.mark.parametrize("mistake", pc.WRONG_UNPACKS)
def test_the_cases_tell_the_model_from_a_wrong_unpack(mistake):
    caught = []
    for name in dc.SHAPES:
        w, h, _ = dc.SHAPES[name]
        for label, lay, new, tiles, rows in pc.unpack_cases(name):
            packed = dc.pack(new, tiles, rows)
            want, _ = pc.unpack_raw(packed, tiles, lay.raw, lay.off, lay.stride, w, h, rows)
            got, _ = pc.unpack_raw(packed, tiles, lay.raw, lay.off, lay.stride, w, h, rows, mistake)
            if (got != want).any():
                caught.append((name, label))
    assert caught, mistake


def test_the_unpack_cases_cover_what_the_issue_names():
    for name, (w, h, _) in dc.SHAPES.items():
        labels = {label for label, _, _, _, _ in pc.unpack_cases(name)}
        for kind in dc.STRIDES:
            for lead in pc.LEADS:
                assert {f"{kind} +{lead} first", f"{kind} +{lead} last", f"{kind} +{lead} all"} <= labels
    lists = pc.tile_lists("many")
    assert len(lists["all but one"]) == 424 and len(lists["65"]) == 65 and dc.pack_geometry(65)[:2] == (64, 2)
    assert (3 * 83) % 8 != 0 and 3 * 83 - 24 * 10 == 9                 # the last tile column of `ragged`: one whole chunk and one byte


# ---- the whole stream, on the CPU, with the oracle ----
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_a_stream_through_the_oracle(ia, oracle, name):
    """the fixtures are self-consistent before a GPU sees them: the expected patches parse, and applying the oracle's decode of each
    patch's container through the model's unpack reproduces the oracle's decode of the whole frame's container, frame after frame"""
    w, h, K = dc.SHAPES[name]
    octx = oracle.OracleContext(K, 8, dc.QUALITY)
    kept, forms = None, set()
    for i, (px, listed, patch) in enumerate(pc.stream(name, lambda p: octx.encode_image(np.ascontiguousarray(p), quant=dc.quant(name)))):
        info = ia.patch_info(patch)
        assert pc.parse(patch)["list"] == ia.patch_tiles(patch).tolist() == (list(range(info["tiles"])) if listed is None else listed)
        assert (info["sequence"], info["key"]) == (i, int(listed is None))
        container = patch[info["container_offset"]:]
        whole = octx.encode_image(np.ascontiguousarray(px), quant=dc.quant(name))
        want = oracle.decode_image(whole)
        if listed is None:
            assert patch == ia.patch_make(w, h, i, None, container, key=True) and container == whole
            kept = want
        elif listed:
            assert patch == ia.patch_make(w, h, i, listed, container)
            kept = pc.unpack(oracle.decode_image(container), listed, kept)
        else:
            assert patch == ia.patch_make(w, h, i, [], None) and len(patch) == 40
        forms.add("key" if listed is None else "tile" if listed else "empty")
        assert (kept == want).all(), (name, i)
    assert "key" in forms and ("tile" in forms) == (pc.tile_count(w, h) > 1) and (name != "full" or "empty" in forms)
    octx.close()
