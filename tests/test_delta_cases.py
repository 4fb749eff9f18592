"""The delta encoder on the host: mpc_changed_tiles and the packed geometry against the numpy model of tests/delta_cases.py on every
case, the cases against the mistakes they are there to catch, refusals, and the declared symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import delta_cases as dc
from conftest import ROOT


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def _host(ia, a, b, block_size=8):
    return ia.changed_tiles(a.pixels, b.pixels, block_size)


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_changed_tiles_is_the_model(ia, name):
    w, h, _ = dc.SHAPES[name]
    for lead in (0, 1):
        for label, a, b in dc.diff_pairs(name, lead):
            assert a.pixels.strides[0] == dc.stride_of(a.kind, w)                # the view keeps its stride: no copy is compared
            want = dc.expected(a, b)
            got = _host(ia, a, b)
            assert got.dtype == np.int32 and (got == want).all() and got.size == want.size, (name, lead, label)
            assert (np.diff(got) > 0).all()
            # two strides in one call, and the frame against itself
            tight = np.ascontiguousarray(a.pixels)
            assert (ia.changed_tiles(tight, b.pixels) == want).all() and ia.changed_tiles(b.pixels, b.pixels).size == 0


def test_the_tile_sets_are_what_they_change():
    for name, (w, h, _) in dc.SHAPES.items():
        px = dc.frame(w, h, 11)
        for label, tiles in dc.tile_sets(name).items():
            assert list(dc.changed_tiles(px, dc.change_tiles(px, tiles, 5))) == sorted(tiles), (name, label)
    tx, ty = dc.grid(*dc.SHAPES["many"][:2])
    assert (tx, ty) == (25, 17) and dc.pack_geometry(tx * ty - 1) == (64, 7, 168, 168 * 512)   # the last packed column partial: 424 = 6 * 64 + 40
    assert dc.grid(83, 45) == (11, 6)


@pytest.mark.parametrize("mistake", dc.WRONG_DIFFS)
def test_the_cases_tell_the_model_from_a_wrong_diff(mistake):
    caught = []
    for name in dc.SHAPES:
        for lead in (0, 1):
            for label, a, b in dc.diff_pairs(name, lead):
                want, got = dc.expected(a, b), dc.wrong_changed_tiles(a, b, mistake)
                if got.size != want.size or (got != want).any():
                    caught.append((name, lead, label))
    assert caught, mistake
    # without a mistake the same function is the model: what it catches is the mistake's
    for label, a, b in dc.diff_pairs("ragged", 1):
        assert (dc.wrong_changed_tiles(a, b, None) == dc.expected(a, b)).all(), label


@pytest.mark.parametrize("mistake", dc.WRONG_PACKS)
def test_the_cases_tell_the_model_from_a_wrong_pack(mistake):
    caught = [(name, label) for name in dc.SHAPES for label, px, tiles, rows in dc.pack_cases(name)
              if (dc.pack(px, tiles, rows, mistake) != dc.pack(px, tiles, rows)).any()]
    assert caught, mistake


def test_the_pack_cases_cover_what_the_issue_names():
    labels = {label for label, _, _, _ in dc.pack_cases("many")}
    for rows in (1, 3, 64):
        for n in {1, rows, rows + 1}:
            assert f"rows {rows} n {n}" in labels
    assert {"all but one", "64", "65", "checkerboard", "unsorted"} <= labels
    # a packed tile is where the tile encoder's own order finds it, and black where the model says
    px = dc.frame(83, 45, 11)
    packed = dc.pack(px, [65, 0, 7], rows=2)
    assert packed.shape == (16, 16, 3)
    assert (packed[8:16, 0:8] == px[0:8, 0:8]).all() and (packed[8:16, 8:16] == 0).all()       # j = 1 at (0, 1); the padding tile
    assert (packed[0:5, 0:3] == px[40:45, 80:83]).all() and (packed[5:8, 0:8] == 0).all() and (packed[0:8, 3:8] == 0).all()


def test_pack_geometry_is_the_model(ia):
    for rows in (1, 3, 64, 1000):
        for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 424, 425, 251328):
            assert ia.delta_pack_geometry(n, rows) == dc.pack_geometry(n, rows), (n, rows)
    R, Cc, stride, nbytes = ia.delta_pack_geometry(65)
    assert (R, Cc, stride, nbytes) == (64, 2, 48, 48 * 512) and stride % 8 == 0 and R * Cc >= 65
    for n, rows in ((-1, 64), (1, 0), (2**31, 64)):
        with pytest.raises(ia.MpcError) as e:
            ia.delta_pack_geometry(n, rows)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT


def test_scatter_model():
    K = 4
    pc, pch = dc.records(3, K, 1)
    counts, choices = dc.records(10, K, 2)
    got_c, got_r, bad = dc.scatter(pc, pch, [7, 10, 0], counts, choices)
    assert bad and (got_c[7] == pc[0]).all() and (got_r[0] == pch[2]).all()
    keep = [t for t in range(10) if t not in (0, 7)]
    assert (got_c[keep] == counts[keep]).all() and (got_r[keep] == choices[keep]).all()


def test_other_block_sizes_compare_the_same_bytes(ia):
    """mpc_changed_tiles takes the block sizes a host-only context takes; the tiles are then smaller, the bytes compared the same"""
    w, h = 13, 9
    a = dc.frame(w, h, 4)
    b = dc.bump(dc.bump(a, 12, 8, 2), 0, 0, 0)
    for bs in range(1, 9):
        ty = -(-h // bs)
        assert list(ia.changed_tiles(a, b, bs)) == [0, (12 // bs) * ty + 8 // bs], bs


def test_refusals(ia):
    L = ia.load_library()
    a = np.zeros((4, 4, 3), np.uint8)
    tiles, n = np.zeros(4, np.int32), C.c_int(-7)
    p, t = a.ctypes.data, tiles.ctypes.data_as(C.POINTER(C.c_int32))

    def call(prev=p, ps=0, cur=p, cs=0, w=4, h=4, bs=8, out=t, count=C.byref(n)):
        return L.mpc_changed_tiles(prev, ps, cur, cs, w, h, bs, out, count)

    assert call() == ia.api.MPC_OK and n.value == 0
    n.value = -7
    for bad in (dict(prev=None), dict(cur=None), dict(out=None), dict(count=None), dict(w=0), dict(h=0), dict(w=-1), dict(bs=0), dict(bs=9),
                dict(ps=11), dict(cs=11), dict(cs=1)):
        assert call(**bad) == ia.api.MPC_ERR_ARGUMENT, bad
        assert L.mpc_last_error()
    assert n.value == -7                                             # a refusal writes nothing
    assert call(ps=12, cs=12) == ia.api.MPC_OK                       # the minimum stride
    # a host-only context: no session, no kernel
    ctx = ia.create_compression_context(4, 8, 3.5)
    with pytest.raises(ia.MpcError) as e:
        ctx.delta_encoder(16, 16)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    for fn, args in ((ctx.tile_diff_device, (8, 8, 8, 8, 0, 8, 8)), (ctx.pack_tiles_device, (8, 8, 8, 0, 8, 1, 64, 8)),
                     (ctx.scatter_records_device, (8, 8, 8, 1, 8, 8, 1))):
        with pytest.raises(ia.MpcError) as e:
            fn(*args)
        assert e.value.status == ia.api.MPC_ERR_NO_DEVICE, fn
    h = C.c_void_p()
    assert L.mpc_delta_create(ctx.h, 0, 8, C.byref(h)) == ia.api.MPC_ERR_ARGUMENT and not h
    assert L.mpc_delta_create(ctx.h, 8, 8, None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_delta_create(None, 8, 8, C.byref(h)) == ia.api.MPC_ERR_ARGUMENT
    L.mpc_delta_destroy(None)                                        # a no-op
    ctx.close()


def test_the_declared_symbols_exist(ia):
    L = ia.load_library()
    text = open(os.path.join(ROOT, "include", "mpcodec.h")).read()
    section = text.split('delta: encode what changed')[1].split('"-s" patch statistics')[0]
    names = set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", section)) - {"mpc_encode_tiles_device", "mpc_encode_image_device", "mpc_container_index2",
                                                                     "mpc_kernel_timing_read", "mpc_crop_records_check", "mpc_compose_indexed",
                                                                     "mpc_encode_image", "mpc_container_index"}
    want = {"mpc_changed_tiles", "mpc_delta_pack_geometry", "mpc_tile_diff_device", "mpc_pack_tiles_device", "mpc_scatter_records_device",
            "mpc_delta_create", "mpc_delta_destroy", "mpc_delta_encode", "mpc_delta_changed"}
    assert want <= names
    for name in want:
        assert hasattr(L, name), name
    for flag, value in (("MPC_DELTA_KEY", 1), ("MPC_DELTA_DEVICE_PIXELS", 2), ("MPC_DELTA_PACK_ALWAYS", 4), ("MPC_DELTA_PACK_ROWS", 64)):
        assert re.search(r"#define %s\s+%du?\b" % (flag, value), section), flag
        assert getattr(ia.api, flag) == value
    assert dc.PACK_ROWS == ia.api.MPC_DELTA_PACK_ROWS
