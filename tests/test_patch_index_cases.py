"""Patch format version 2 on the host: the library's writer, parsers, add and strip (mpc_patch_make_indexed, mpc_patch_info,
mpc_patch_tiles, mpc_patch_index, mpc_patch_add_index, mpc_patch_strip_index) against the pure-Python model of
tests/patch_index_cases.py, the version-2 blobs every parser must refuse, the version-1 corpus of tests/patch_cases.py refused as
before, and the precondition of the device tests: every container-and-index pair they use is one the host's chunked parse accepts.
No GPU.  Every equality is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import delta_cases as dc
import patch_cases as pc
import patch_index_cases as pic
from conftest import ROOT


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def blank_container(ia, w, h, K=8):
    """a valid container of w x h pixels made on the host: every tile-channel of length 0"""
    tiles = pc.tile_count(w, h)
    return ia.assemble_streams(w, h, K, 8, ia.quant_tables(K, dc.QUALITY), np.zeros((tiles, 3), np.uint16), np.zeros((tiles, 3, K), np.uint32))


def filled_container(ia, w, h, K=8, seed=1):
    """one with records in it: hand-made counts and words (delta_cases.records), so that every stream has symbols"""
    counts, choices = dc.records(pc.tile_count(w, h), K, seed)
    return ia.assemble_streams(w, h, K, 8, ia.quant_tables(K, dc.QUALITY), counts, choices)


def packed_container(ia, n, filled=True):
    R, Cc, _, _ = dc.pack_geometry(n)
    return filled_container(ia, 8 * Cc, 8 * R, seed=n) if filled else blank_container(ia, 8 * Cc, 8 * R)


def _agree(ia, w, h, sequence, tiles, container, key=False, index=None):
    """the library's writer gives the model's bytes, and the parsers read them alike: info and tiles as for the stripped patch"""
    want = pic.make(w, h, sequence, tiles, container, key, index)
    got = ia.patch_make(w, h, sequence, tiles, container, key, index=index)
    assert got == want, (w, h, sequence, key)
    model = pic.parse(got)
    listed = model.pop("list")
    version, at, size = model.pop("version"), model.pop("index_offset"), model.pop("index_bytes")
    assert version == (2 if index else 1) and size == len(index or b"")
    assert ia.patch_info(got) == model == ia.patch_info(pic.strip(got))
    assert ia.patch_tiles(got).tolist() == listed == ia.patch_tiles(pic.strip(got)).tolist()
    assert ia.patch_index(got) == (at, size)
    assert got[at:at + size] == (index or b"") and (not index or at + size == len(got))
    assert ia.patch_strip_index(got) == pic.strip(got) == pc.make(w, h, sequence, tiles, container, key)
    return got


def test_the_writer_and_the_parsers_are_the_model(ia):
    for name in ("ragged", "many", "full", "one"):
        w, h, K = dc.SHAPES[name]
        all_tiles = pc.tile_count(w, h)
        whole = filled_container(ia, w, h, K)
        for interval in pic.INTERVALS:
            index = ia.container_index(whole, interval)
            key = _agree(ia, w, h, 4, None, whole, key=True, index=index)
            assert ia.patch_info(key)["key"] == 1 and ia.patch_tiles(key).tolist() == list(range(all_tiles))
        _agree(ia, w, h, 4, None, whole, key=True)                                  # no index: the version-1 blob
        _agree(ia, w, h, 4, None, whole, key=True, index=b"")
        for label, listed in pc.tile_lists(name).items():
            if len(listed) == all_tiles:
                continue
            cont = packed_container(ia, len(listed))
            index = ia.container_index(cont, 32)
            # the list's length moves the section over every alignment; the bytes are the writer's concern, not their meaning
            for section in (index, index[:-3], b"x", bytes(range(256)) * 3):
                _agree(ia, w, h, 2**32 - 1, listed, cont, index=section)
    # offsets of the index section cover all 8 alignments
    w, h, _ = dc.SHAPES["many"]
    seen = set()
    for n in range(1, 12):
        cont = packed_container(ia, n, filled=False)
        seen.add(ia.patch_index(ia.patch_make(w, h, 0, list(range(0, 30 * n, 30)), cont, index=b"abc"))[0] % 8)
        seen.add(ia.patch_index(ia.patch_make(w, h, 0, list(range(n)), filled_container(ia, 8, 8 * n, seed=n), index=b"abc"))[0] % 8)
    assert seen == set(range(8)), seen


def _stream(ia, oracle, name):
    w, h, K = dc.SHAPES[name]
    octx = oracle.OracleContext(K, 8, dc.QUALITY)
    out = pic.stream(name, lambda p: octx.encode_image(np.ascontiguousarray(p), quant=dc.quant(name)))
    octx.close()
    return out


@pytest.fixture(scope="module")
def real(ia, oracle):
    """the oracle's stream of `ragged`: real containers, the first and the next tile patch among them"""
    return _stream(ia, oracle, "ragged")


def test_add_and_strip_are_the_model(ia, real):
    w, h, _ = dc.SHAPES["ragged"]
    host = [ia.patch_make(w, h, 9, [5, 40], packed_container(ia, 2)), ia.patch_make(w, h, 9, None, filled_container(ia, w, h), key=True),
            ia.patch_make(w, h, 9, None, blank_container(ia, w, h), key=True), ia.patch_make(w, h, 9, [], None)]
    forms = set()
    for patch in host + [p for _, _, p in real]:
        info = ia.patch_info(patch)
        cb = info["container_bytes"]
        for interval in pic.INTERVALS:
            want = pic.add_index(patch, interval)
            got = ia.patch_add_index(patch, interval)
            assert got == want
            assert pic.parse(got)["version"] == (2 if info["n"] else 1)
            assert ia.patch_strip_index(got) == patch == pic.strip(got)
            assert ia.patch_info(got) == info and ia.patch_tiles(got).tolist() == ia.patch_tiles(patch).tolist()
            # an already indexed patch: the index is replaced, whatever it was
            assert ia.patch_add_index(got, interval) == got
            assert ia.patch_add_index(ia.patch_add_index(patch, 64), interval) == got
            assert ia.patch_strip_index(ia.patch_strip_index(got)) == patch
            if info["n"]:
                at, size = ia.patch_index(got)
                container = patch[info["container_offset"]:]
                assert got[at:] == ia.container_index(container, interval) and size == len(got) - at
                assert ia.patch_add_index(pic.make(w, h, info["sequence"], ia.patch_tiles(patch), container, bool(info["key"]), b"garbage"), interval) == got
                # index_min_bytes on both sides of the boundary
                assert ia.patch_add_index(patch, interval, cb) == got == pic.add_index(patch, interval, cb)
                assert ia.patch_add_index(patch, interval, cb + 1) == patch == pic.add_index(patch, interval, cb + 1)
                assert ia.patch_add_index(got, interval, cb + 1) == patch                # stripped, and left at version 1
                assert ia.patch_add_index(patch, interval, 1) == got and ia.patch_add_index(patch, interval, 2**63) == patch
            else:
                assert got == patch and len(got) == 40 and ia.patch_index(got) == (0, 0)
        forms.add("key" if info["key"] else "tile" if info["n"] else "empty")
    assert forms == {"key", "tile", "empty"}
    # a container whose header reads and whose streams do not: no index can be built, the patch stays at version 1
    patch = next(p for _, listed, p in real if listed)
    info = ia.patch_info(patch)
    broken = bytearray(patch)
    broken[info["container_offset"] + 24 + 3 * 8 * 2:] = b"\xff" * (len(patch) - info["container_offset"] - 24 - 3 * 8 * 2)
    broken = bytes(broken)
    ia.patch_info(broken)
    with pytest.raises(ia.MpcError):
        ia.container_index(broken[info["container_offset"]:], 32)
    assert ia.patch_add_index(broken, 32) == broken == pic.add_index(broken, 32)
    # the interval's rules are mpc_container_index's
    for bad in (1, 31, 65537, -1):
        with pytest.raises(ia.MpcError) as e:
            ia.patch_add_index(patch, bad)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT


def _valid(ia, real):
    w, h, _ = dc.SHAPES["ragged"]
    tile = next(p for _, listed, p in real if listed and len(listed) >= 2)
    key = real[0][2]
    empty = ia.patch_make(w, h, 9, [], None)
    return ia.patch_add_index(tile, 32), ia.patch_add_index(key, 32), empty


def _refusal_writes_nothing(ia, L, blob, label):
    info, n, at, size = ia.api.MpcPatchInfo(), C.c_int(-7), C.c_size_t(77), C.c_size_t(78)
    out, nb = C.POINTER(C.c_uint8)(), C.c_size_t(79)
    S = ia.api.MPC_ERR_BITSTREAM
    before = bytes(info)
    buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")           # an exact-size buffer of its own
    assert L.mpc_patch_info(buf, len(blob), C.byref(info)) == S, label
    assert L.mpc_last_error()
    assert L.mpc_patch_tiles(buf, len(blob), None, 0, C.byref(n)) == S, label
    assert L.mpc_patch_index(buf, len(blob), C.byref(at), C.byref(size)) == S, label
    assert L.mpc_patch_strip_index(buf, len(blob), C.byref(out), C.byref(nb)) == S, label
    assert L.mpc_patch_add_index(buf, len(blob), 32, 0, C.byref(out), C.byref(nb)) == S, label
    assert bytes(info) == before and (n.value, at.value, size.value, nb.value) == (-7, 77, 78, 79) and not out, label


def test_hostile_version_2_blobs_are_refused(ia, real):
    L = ia.load_library()
    tile, key, empty = _valid(ia, real)
    for good in (tile, key, empty):
        ia.patch_info(good)
        pic.parse(good)
    cases = pic.hostile(tile, key, empty)
    labels = {label for label, _ in cases}
    assert {"tile: index_bytes 0", "key: index_bytes 0", "tile: one byte short", "tile: one byte long", "key: one byte short", "key: one byte long",
            "version 2 with n = 0", "version 2 with an index on an empty form", "tile: version 1 with index_bytes set",
            "key: version 1 with index_bytes set"} <= labels
    assert sum(label.startswith("prefix ") for label in labels) == len(tile)
    for label, blob in cases:
        with pytest.raises(pc.Refused):
            pic.parse(blob)
        _refusal_writes_nothing(ia, L, blob, label)


def test_the_version_1_corpus_is_still_refused(ia):
    """patch_cases.hostile, imported as it is: "wrong version" -- a version-1 tile patch whose version word says 2 -- among them"""
    L = ia.load_library()
    w, h, _ = dc.SHAPES["ragged"]
    tile = ia.patch_make(w, h, 9, [5, 40], packed_container(ia, 2, filled=False))
    key = ia.patch_make(w, h, 9, None, blank_container(ia, w, h), key=True)
    empty = ia.patch_make(w, h, 9, [], None)
    cases = pc.hostile(tile, key, empty, blank_container(ia, 8, 24))
    assert "wrong version" in {label for label, _ in cases} and "a nonzero reserved word" in {label for label, _ in cases}
    for label, blob in cases:
        with pytest.raises(pc.Refused):
            pic.parse(blob)
        _refusal_writes_nothing(ia, L, blob, label)
    # and every valid version-1 patch reads as before
    for good in (tile, key, empty):
        assert ia.patch_info(good) == {k: v for k, v in pc.parse(good).items() if k != "list"} and ia.patch_index(good) == (0, 0)
        assert ia.patch_strip_index(good) == good


def test_argument_refusals(ia, real):
    L, A = ia.load_library(), ia.api.MPC_ERR_ARGUMENT
    w, h, _ = dc.SHAPES["ragged"]
    cont = packed_container(ia, 2)
    index = ia.container_index(cont, 32)
    with pytest.raises(ia.MpcError) as e:
        ia.patch_make(w, h, 0, [], None, index=index)                               # an index for an empty patch
    assert e.value.status == A
    for bad in (dict(tiles=[40, 5]), dict(container=None), dict(w=0), dict(key=True, container=None)):
        v = dict(dict(w=w, tiles=[5, 40], container=cont, key=False), **bad)
        with pytest.raises(ia.MpcError) as e:
            ia.patch_make(v["w"], h, 0, v["tiles"], v["container"], v["key"], index=index)
        assert e.value.status == A, bad
    tile = ia.patch_add_index(ia.patch_make(w, h, 0, [5, 40], cont), 32)
    buf = (C.c_uint8 * len(tile)).from_buffer_copy(tile)
    cbuf = (C.c_uint8 * len(cont)).from_buffer_copy(cont)
    listed = np.asarray([5, 40], np.int32)
    lp = listed.ctypes.data_as(C.POINTER(C.c_int32))
    out, nb, at, size = C.POINTER(C.c_uint8)(), C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
    # index_bytes of 2^32 and more: refused before a byte of it is read; a null index with a size
    assert L.mpc_patch_make_indexed(w, h, 0, 0, lp, 2, cbuf, len(cont), cbuf, 2**32, C.byref(out), C.byref(nb)) == A and not out
    assert L.mpc_patch_make_indexed(w, h, 0, 0, lp, 2, cbuf, len(cont), None, 8, C.byref(out), C.byref(nb)) == A and not out
    assert L.mpc_patch_make_indexed(w, h, 0, 0, lp, 2, cbuf, len(cont), cbuf, 8, None, C.byref(nb)) == A
    assert L.mpc_patch_make_indexed(w, h, 0, 0, lp, 2, cbuf, len(cont), cbuf, 8, C.byref(out), None) == A
    assert L.mpc_patch_index(None, len(tile), C.byref(at), C.byref(size)) == A
    assert L.mpc_patch_index(buf, len(tile), None, C.byref(size)) == A and L.mpc_patch_index(buf, len(tile), C.byref(at), None) == A
    assert L.mpc_patch_add_index(None, len(tile), 32, 0, C.byref(out), C.byref(nb)) == A
    assert L.mpc_patch_add_index(buf, len(tile), 32, 0, None, C.byref(nb)) == A and L.mpc_patch_add_index(buf, len(tile), 32, 0, C.byref(out), None) == A
    assert L.mpc_patch_strip_index(None, len(tile), C.byref(out), C.byref(nb)) == A
    assert L.mpc_patch_strip_index(buf, len(tile), None, C.byref(nb)) == A and L.mpc_patch_strip_index(buf, len(tile), C.byref(out), None) == A
    assert (nb.value, at.value, size.value) == (7, 7, 7) and not out
    assert L.mpc_patch_last_route(None) == -1
    # a host-only context has no sender
    ctx = ia.create_compression_context(4, 8, 3.5)
    with pytest.raises(ia.MpcError) as e:
        ctx.delta_encoder(16, 16)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    ctx.close()


def test_the_declared_symbols_exist(ia):
    L = ia.load_library()
    text = open(os.path.join(ROOT, "include", "mpcodec.h")).read()
    section = text.split("patch index: a patch that carries its container's seek index")[1].split("test entry points")[0].split("*/", 1)[1]
    names = set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", section, flags=re.S)))
    want = {"mpc_patch_index", "mpc_patch_make_indexed", "mpc_patch_add_index", "mpc_patch_strip_index", "mpc_delta_encode_patch_indexed",
            "mpc_patch_last_route"}
    assert names == want, names ^ want
    for name in want:
        assert hasattr(L, name), name
    for name in ("patch_index", "patch_add_index", "patch_strip_index"):
        assert hasattr(ia, name)
    assert hasattr(ia.PatchDecoder, "last_route")
    # without index_interval the encoders behave as before; the default of index_min_bytes is the measured size (profiles/patch_index.txt)
    import inspect
    for call in (ia.DeltaEncoder.encode_patch, ia.DeltaEncoder.encode_patch_device):
        p = inspect.signature(call).parameters
        assert p["index_interval"].default is None and p["index_min_bytes"].default == ia.api.PATCH_INDEX_MIN_BYTES == 12134
    # struct mpc_patch_info and Python's dict are what they were
    assert [f for f, _ in ia.api.MpcPatchInfo._fields_] == ["width", "height", "sequence", "key", "n", "tiles", "container_offset", "container_bytes"]


# ---- the precondition of the device tests ----
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_every_pair_of_the_device_tests_takes_route_0(ia, oracle, name):
    """not a measurement: for every container the device tests send, at both of their intervals, the host's chunked parse accepts
    container_index's blob (route 0) and yields the serial parse's symbols -- so a device test that asserts route 0 cannot hide an index
    that was quietly refused.  The containers are the oracle's, byte for byte the device encoder's by the parity tests"""
    w, h, K = dc.SHAPES[name]
    forms, chunks = set(), set()
    for i, (px, listed, patch) in enumerate(_stream(ia, oracle, name)):
        info = ia.patch_info(patch)
        assert info["sequence"] == i and pc.parse(patch)["list"] == (list(range(info["tiles"])) if listed is None else listed)
        forms.add("key" if listed is None else "tile" if listed else "empty")
        if not info["n"]:
            continue
        container = patch[info["container_offset"]:]
        serial = ia.read_compressed(container, coded=True)
        for interval in pic.INTERVALS:
            index = ia.container_index(container, interval)
            assert ia.index_version(index) == 1 and not ia.index_info(index)["serial_only"]
            symbols, route = ia.parse_container_by_index(container, index)
            assert route == 0, (name, i, interval)
            want = np.concatenate([np.asarray(serial["lengths"], np.uint16).reshape(-1)] + [np.asarray(c, np.uint16) for c in serial["codes"]])
            assert (symbols == want).all()
            assert ia.patch_add_index(patch, interval) == pic.make(w, h, i, listed, container, listed is None, index)
            if interval == 32:
                chunks.add(len(ia.index_info(index)["streams"][0]["checkpoints"]))
    assert "key" in forms and "empty" in forms and ("tile" in forms) == (pc.tile_count(w, h) > 1)
    if name == "many":
        # the lengths stream has 3 symbols a tile of the container's own frame: the key patch's 425 tiles give 1275, 40 chunks with the
        # last one short; the 424 listed tiles lie in a packed frame of 64 x 7 = 448, 1344 symbols, 42 whole chunks
        assert {40, 42} <= chunks and 3 * 425 % 32 != 0 and 3 * 448 % 32 == 0
    if name == "one":
        assert chunks == {1}                                                       # the one-chunk case
