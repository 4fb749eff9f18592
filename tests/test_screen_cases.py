"""The pursuit screen's host side, without a device: mpc_filter_tiles (the function that makes the split-bf16 filter tiles the
pursuit kernel reads) against a restatement of bfloat16 rounding and of the operand layout of DESIGN.md 3, and the inputs of
test_gpu_screen_tables.py against a numpy model of the screen -- they are fair (the model stays inside the bound E_b on every one
of them) before a GPU sees them.

Worst |model - exact| / E_b per class (rows: the 510 base rows and blocks 0, 1, 509 of the three channels): gaussian 0.023,
pixels 0.012, huge_projection 0.050, magnitudes 0.052, bf16_midpoints 0.047, subnormal 1.3e-10, near_huge 0.023, constant 0.060,
with_zero 0.032."""
import ctypes as C

import numpy as np
import pytest

import screen_cases as sc


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd
    return imageexperiments_amd


@pytest.fixture(scope="module")
def dic(octx32):
    """the oracle's dictionary: base[510,64], block_rows[510], detail[3][31622,64], first detail row of every block"""
    rows = np.asarray(octx32.det_rows, np.int64)
    return octx32.base, rows, [octx32.det[ch] for ch in range(3)], sc.row_offsets(rows)


def block_of(dic, ch, blk):
    _, rows, det, off = dic
    return det[ch][off[blk]:off[blk] + rows[blk]]


def test_dictionary_facts_the_sample_rests_on(dic):
    base, rows, det, off = dic
    assert base.shape == (sc.NUM_BASE, 64) and off[-1] == 31622 and all(d.shape == (31622, 64) for d in det)
    assert (base[509].view(np.uint64) == (-base[0]).view(np.uint64)).all()
    assert rows[0] == 63 and rows[509] == 63 and (rows[1:509] == 62).all()
    assert not (det[0] == det[1]).all() and not (det[1] == det[2]).all() and not (det[0] == det[2]).all()
    n_sel = sc.NUM_BASE + int(off[-1])
    assert n_sel == 502 * 64 + 4
    tiles = sc.sample_selector_tiles(n_sel)
    assert len(set(tiles)) == 11 and tiles[:3] == [0, 7, 502] and 7 * 64 <= 509 < 510 < 8 * 64
    assert len(set(sc.sample_blocks())) == 8 and sc.sample_blocks()[:4] == [0, 1, 509, 255]


def check_tiles(ia, rows, tiles, k_order, want_shadow):
    """every stored pair of mpc_filter_tiles(rows) decoded through the documented layout: values, positions, zero rows"""
    rows = np.asarray(rows, np.float64).reshape(-1, 64)
    n = rows.shape[0]
    out, shadow = ia.api.filter_tiles(rows, tiles, k_order)
    assert out.shape == (tiles * sc.TILE_HALVES,)
    assert shadow.tolist() == list(want_shadow)
    hi, lo = sc.decode_tiles(out, tiles, k_order)                  # by (row, pixel); the layout covers every element once
    want_hi, want_lo = sc.split_bf16(rows)
    kept = np.asarray(want_shadow) == 0
    assert (hi[:n][kept] == want_hi[kept]).all()                     # hi = bf16(float32(x)), nearest even, where DESIGN.md 3 puts it
    assert (lo[:n][kept] == want_lo[kept]).all()                     # lo = bf16(float32(x) - hi)
    assert not hi[:n][~kept].any() and not lo[:n][~kept].any()       # shadowed rows: all-zero halves
    assert not hi[n:].any() and not lo[n:].any()                     # rows >= nrows: all-zero halves
    x = rows[kept]
    rest = x - sc.bf16_value(hi[:n][kept]).astype(np.float64) - sc.bf16_value(lo[:n][kept]).astype(np.float64)      # exact in double
    assert (np.abs(rest) <= 2.0 ** -16 * np.abs(x)).all()            # the premise of the bound


@pytest.mark.parametrize("k_order", [1, 0])
def test_filter_tiles_of_the_base_rows(ia, dic, k_order):
    want = np.zeros(sc.NUM_BASE, np.uint8)
    want[509] = 1                                                    # bit for bit -row 0: exactly this row is shadowed
    check_tiles(ia, dic[0], 32, k_order, want)


@pytest.mark.parametrize("k_order", [1, 0])
@pytest.mark.parametrize("blk", [0, 1, 509])
@pytest.mark.parametrize("ch", [0, 1, 2])
def test_filter_tiles_of_detail_blocks(ia, dic, ch, blk, k_order):
    rows = block_of(dic, ch, blk)
    check_tiles(ia, rows, 4, k_order, np.zeros(rows.shape[0], np.uint8))      # nothing in a detail block is shadowed


def test_k_orders_differ_and_k_order_1_is_the_pursuit_layout(ia, dic):
    """Lane (row & 15, h) of k order 1 holds 16 consecutive pixels 16 pos(h) .. + 15 over its two operands; k order 0 does not."""
    out1, _ = ia.api.filter_tiles(dic[0], 32, 1)
    out0, _ = ia.api.filter_tiles(dic[0], 32, 0)
    assert not (out1 == out0).all()
    p1 = sc.operand_pixels(1)
    for lane in range(64):
        got = sorted(p1[0, lane].tolist() + p1[1, lane].tolist())
        assert got == list(range(16 * sc.POS[lane >> 4], 16 * sc.POS[lane >> 4] + 16))


@pytest.mark.parametrize("tiles", [1, 2, 3, 4])
@pytest.mark.parametrize("nrows", [1, 15, 17, 62])
def test_filter_tiles_of_synthetic_rows(ia, nrows, tiles):
    """Planted among random rows (nrows >= 15): the last row duplicates row 2, the one before it is -row 5 (both across a tile
    boundary for 17 and 62 rows), the third from the end is row 1 with the sign of its one zero element flipped, the fourth from
    the end is -row 1 (its zero negated as well).
    What the function does with the sign of a zero, pinned here: it compares bit patterns, so row 1 with only a zero's sign flipped
    is NEITHER a duplicate NOR a negation and keeps its own filter copy (harmless: the exact evaluation, where it ties with row 1,
    decides, and Select()'s strict '>' keeps the earlier row), while the bit-for-bit negation, zero included, is shadowed.  The
    Gram kernel reads the very array this function returns, so the two cannot disagree about such a row."""
    if nrows > 16 * tiles:
        with pytest.raises(ia.MpcError) as e:
            ia.api.filter_tiles(np.ones((nrows, 64)), tiles, 1)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
        return
    rng = np.random.default_rng(100 * nrows + tiles)
    rows = rng.standard_normal((nrows, 64)) * 10.0 ** rng.uniform(-3, 3, (nrows, 1))
    want = np.zeros(nrows, np.uint8)
    if nrows >= 15:
        rows[1, 10] = 0.0
        rows[nrows - 1] = rows[2]
        rows[nrows - 2] = -rows[5]
        rows[nrows - 3] = rows[1]
        rows[nrows - 3, 10] = -0.0
        rows[nrows - 4] = -rows[1]
        assert np.signbit(rows[nrows - 3, 10]) and np.signbit(rows[nrows - 4, 10]) and not np.signbit(rows[1, 10])
        want[[nrows - 1, nrows - 2, nrows - 4]] = 1
    for k_order in (1, 0):
        check_tiles(ia, rows, tiles, k_order, want)


def test_filter_tiles_refusals(ia):
    L = ia.load_library()
    rows = np.ones((16, 64))
    out = np.zeros(sc.TILE_HALVES, np.uint16)
    dp, u16p = C.POINTER(C.c_double), C.POINTER(C.c_uint16)
    A = ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_filter_tiles(None, 16, 1, 1, out.ctypes.data_as(u16p), None) == A
    assert L.mpc_filter_tiles(rows.ctypes.data_as(dp), 16, 1, 1, None, None) == A
    for nrows, tiles, k_order in ((17, 1, 1), (-1, 1, 1), (16, 0, 1), (16, 65, 1), (16, 1, 2), (16, 1, -1)):
        assert L.mpc_filter_tiles(rows.ctypes.data_as(dp), nrows, tiles, k_order, out.ctypes.data_as(u16p), None) == A
    assert not out.any()
    assert L.mpc_filter_tiles(rows.ctypes.data_as(dp), 16, 1, 1, out.ctypes.data_as(u16p), None) == ia.api.MPC_OK      # shadow is optional
    assert out.any()


def test_debug_entries_refuse_a_host_only_context(ia):
    """no device: MPC_ERR_NO_DEVICE from every entry that takes a context (null context: MPC_ERR_ARGUMENT), before anything else"""
    ctx = ia.create_compression_context(8, 8, 3.5, device=-1)
    for call in (lambda: ctx.debug_copy_gram_device(0, 0, 1, 0, 1, 4096),
                 lambda: ctx.debug_copy_filter_tiles(-1),
                 lambda: ctx.debug_copy_filter_tiles(0, 0),
                 lambda: ctx.debug_screen_probe_device(0, 0, 4096, 1, 4096, 4096)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    L = ia.load_library()
    assert L.mpc_debug_copy_gram_device(None, 0, 0, 1, 0, 1, 4096, None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_debug_copy_filter_tiles(None, -1, 0, np.zeros(4, np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_debug_screen_probe_device(None, 0, 0, 4096, 1, 4096, 4096, None) == ia.api.MPC_ERR_ARGUMENT
    with pytest.raises(ia.MpcError) as e:                                      # null pointers are refused before a device is looked for
        ia.api.debug_gram_device(0, 4096, 4096, 4096, 4096, 3, 130, 4096)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    ctx.close()


def test_synthetic_dictionary_is_what_the_gram_test_needs(ia):
    base, detail, rows, off, shadow = sc.synthetic_dictionary()
    assert rows.tolist() == [64, 62, 1] and off.tolist() == [0, 64, 126] and sc.SYN_N_SEL == 130 == 2 * 64 + 2
    assert np.allclose((base * base).sum(axis=1), 1.0, atol=1e-15) and np.allclose((detail * detail).sum(axis=1), 1.0, atol=1e-15)
    assert np.nonzero(shadow)[0].tolist() == [40, 64 + 30]
    for b in range(3):                                   # the planted flags are the ones mpc_filter_tiles finds in each block
        _, sh = ia.api.filter_tiles(detail[off[b]:off[b] + rows[b]], 4, 1)
        assert (sh == shadow[off[b]:off[b] + rows[b]]).all()


@pytest.mark.parametrize("name", sc.CLASSES)
def test_model_of_the_screen_stays_inside_the_bound(dic, name):
    """|model approximation - exact projection| <= E_b on every class, for the base rows and blocks 0, 1, 509 of every channel"""
    base = dic[0]
    rows = np.concatenate([base] + [block_of(dic, ch, blk) for ch in range(3) for blk in (0, 1, 509)])
    v = sc.residual_class(name, base)
    assert v.shape == (16, 64) and np.isfinite(v.astype(np.float32)).all()
    approx = sc.model_screen(rows, v).astype(np.longdouble)
    exact = sc.exact_products(v, rows)
    bound = sc.model_bound(v).astype(np.longdouble)
    ratio = np.abs(approx - exact) / bound[:, None]
    print(f"screen model, class {name}: worst |approx - exact| / E_b = {float(ratio.max()):.3g}")
    assert (ratio <= 1).all()
    # what makes the class what it is
    x32 = v.astype(np.float32)
    norm = np.sqrt((x32.astype(np.float64) ** 2).sum(axis=1))
    assert (norm < 1.0e30).all()                                               # the screen is not skipped (kHuge)
    if name == "subnormal":
        assert (np.abs(x32[x32 != 0]) < np.finfo(np.float32).tiny).any() and (bound < 2 * sc.K_ABS).all()
    if name == "near_huge":
        assert (norm > 1.0e28).all()
    if name == "bf16_midpoints":
        hi, lo = sc.split_bf16(v)
        assert (v == x32).all() and (np.abs(sc.bf16_value(lo)) == np.abs(x32) / 257.0).all() and not (hi & 1).any()
    if name == "huge_projection":
        assert (np.abs(exact[:, :sc.NUM_BASE]).max(axis=1) > 999.0).all()
    if name == "constant":
        assert (v == v[:, :1]).all()
    if name == "with_zero":
        assert not v[sc.ZERO_SLOT].any() and (approx[sc.ZERO_SLOT] == 0).all() and v[np.arange(16) != sc.ZERO_SLOT].any(axis=1).all()
