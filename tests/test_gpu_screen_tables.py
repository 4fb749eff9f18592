"""The pursuit screen's device-side tables, read back and probed: the Gram table (mp_gram_kernel), the uploaded split-bf16 filter
tiles, and the bound E_b of the MFMA approximations.  None of them decides a record, so the bit-parity tests
cannot see them wrong; here each is held to a long double (or, for the whole table, float64) reference.

The probe (mpc_debug_screen_probe_device) runs the pursuit kernel's own operand split, bound and six-MFMA tile product
(screen_operands, tile_mfma in mp_pursuit.hip, shared by both kernels) on the resident tiles.

Base row 509 is bit for bit -row 0 and has no filter copy (its approximation is exactly 0, and it can never be returned: it ties
with row 0).  The bound therefore is asserted for base rows 0 .. 508 and the block's real rows; for row 509 the test asserts the
zero and the exact tie instead.

Measured on an MI355X, worst |approx - exact| / E_b per class over blocks 0, 1, 509 of the three channels (also in DESIGN.md 3):
gaussian 0.023, pixels 0.012, huge_projection 0.051, magnitudes 0.053, bf16_midpoints 0.046, subnormal 1.3e-10, near_huge 0.023,
constant 0.060, with_zero 0.033.  No threshold tighter than 1 is asserted: the matrix cores' accumulation order is not documented.
The whole-table comparison takes 0.04 to 0.5 s per channel there."""
import time

import numpy as np
import pytest

import screen_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
N_COLS = sc.NUM_BASE * 64


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd
    return imageexperiments_amd


@pytest.fixture(scope="module")
def ctx(ia, torch):
    c = ia.create_compression_context(32, 8, 3.5, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dic(ctx):
    base, rows, det = ctx.dictionary()
    rows = rows.astype(np.int64)
    return base, rows, det, sc.row_offsets(rows)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gram_rect(torch, ctx, ch, sel_begin, sel_count, col_begin=0, col_count=N_COLS):
    out = torch.full((sel_count, col_count), SENTINEL, dtype=torch.float32, device="cuda")
    ctx.debug_copy_gram_device(ch, sel_begin, sel_count, col_begin, col_count, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- Gram, small: the kernel on a synthetic dictionary ----------------------------------------------------------
def test_gram_kernel_on_the_synthetic_dictionary(ia, torch):
    base, detail, rows, off, shadow = sc.synthetic_dictionary()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (base, detail, rows, off, shadow)]
    stride = sc.SYN_NUM_BASE * 64
    g = torch.full((3 * 64, stride), SENTINEL, dtype=torch.float32, device="cuda")       # three selector tiles; n_sel = 130 of 192 rows
    ia.api.debug_gram_device(*[d.data_ptr() for d in dev], sc.SYN_NUM_BASE, sc.SYN_N_SEL, g.data_ptr())
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    assert (g[sc.SYN_N_SEL:] == SENTINEL).all()                        # rows sel >= n_sel of the last tile are never written
    sel = np.concatenate([base, detail])
    real = np.zeros(stride, bool)
    for blk in range(sc.SYN_NUM_BASE):
        cols = np.zeros((64, 64))
        keep = np.arange(rows[blk])[shadow[off[blk]:off[blk] + rows[blk]] == 0]
        cols[keep] = detail[off[blk] + keep]
        real[64 * blk + keep] = True
        ref = sc.exact_products(sel, cols)
        bad = sc.gram_violations(g[:sc.SYN_N_SEL, 64 * blk:64 * blk + 64], ref)
        assert not bad.any(), (blk, np.argwhere(bad)[:5])
    assert real.sum() == 64 + 62 + 1 - 2
    assert (bits(g[:sc.SYN_N_SEL][:, ~real]) == 0).all()               # pad rows and shadowed rows: exactly +0.0f
    assert (g[:sc.SYN_N_SEL][:, real] != 0).all()


# ---- Gram, resident, sampled -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [0, 1, 2])
def test_resident_gram_sample_against_long_double(torch, ctx, dic, ch):
    """every (selector tile, block) of the sample, the reference written from what the pursuit's `resolve` means by a selector"""
    base, rows, det, off = dic
    n_sel = sc.NUM_BASE + int(off[-1])
    blocks = sc.sample_blocks()
    cols = np.concatenate([sc.block_columns(det[ch], rows, b) for b in blocks])
    for tile in sc.sample_selector_tiles(n_sel):
        s0, s1 = 64 * tile, min(64 * tile + 64, n_sel)
        band = gram_rect(torch, ctx, ch, s0, s1 - s0)
        ref = sc.exact_products(sc.selector_rows(base, det[ch], s0, s1), cols)
        for i, b in enumerate(blocks):
            got = band[:, 64 * b:64 * b + 64]
            bad = sc.gram_violations(got, ref[:, 64 * i:64 * i + 64])
            assert not bad.any(), (tile, b, np.argwhere(bad)[:5])
            assert (bits(got[:, rows[b]:]) == 0).all(), (tile, b)      # pad columns


@pytest.mark.parametrize("ch", [0, 1, 2])
def test_resident_gram_row_509_negates_row_0(torch, ctx, dic, ch):
    _, rows, _, _ = dic
    g0 = gram_rect(torch, ctx, ch, 0, 1)[0]
    g509 = gram_rect(torch, ctx, ch, 509, 1)[0]
    pad = (np.arange(N_COLS) % 64) >= np.repeat(rows, 64)
    # bit for bit, for every entry that is not zero.  A product that is exactly zero (row 0 is the constant row, and a detail row
    # may sum to nothing) is +0.0f in BOTH rows: the kernel's chain starts from +0.0 and x + (-x) rounds to +0, so no -0 arises.
    nz = g0 != 0
    assert (bits(g509[nz]) == bits(-g0[nz])).all()
    assert (bits(g509[~nz]) == 0).all() and (bits(g0[~nz]) == 0).all()
    assert not nz[pad].any() and nz[~pad].sum() > nz.size // 2


@pytest.mark.parametrize("ch", [0, 1, 2])
def test_resident_gram_diagonal_and_symmetry(torch, ctx, dic, ch):
    """G[510 + off_a + i][64 b + j] == G[510 + off_b + j][64 a + i] bit for bit (the same products in the same k order), and a
    block against itself has a diagonal within 2^-23 of 1"""
    _, rows, _, off = dic
    blocks = sc.sample_blocks()
    bands = {a: gram_rect(torch, ctx, ch, sc.NUM_BASE + int(off[a]), int(rows[a])) for a in blocks}
    for a in blocks:
        diag = np.diagonal(bands[a][:, 64 * a:64 * a + rows[a]]).astype(np.float64)
        assert (np.abs(diag - 1.0) <= 2.0 ** -23).all(), a
        for b in blocks:
            ab = bands[a][:, 64 * b:64 * b + rows[b]]                   # [i, j]
            ba = bands[b][:, 64 * a:64 * a + rows[a]]                   # [j, i]
            assert (bits(ab) == bits(ba.T)).all(), (a, b)


# ---- Gram, resident, whole ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [0, 1, 2])
def test_resident_gram_whole_table_against_float64(torch, ctx, dic, ch):
    """All 32 132 x 32 640 entries of a channel against a float64 matrix product on the device: what finds a missing or misplaced
    tile anywhere.  2^-24 relative (G's one rounding) + 2^-45 absolute (the library's own summation order over 64 terms)."""
    base, rows, det, off = dic
    n_sel = sc.NUM_BASE + int(off[-1])
    src = np.full(N_COLS, -1, np.int64)                                # column -> detail row, -1 for a pad
    for b in range(sc.NUM_BASE):
        src[64 * b:64 * b + rows[b]] = off[b] + np.arange(rows[b])
    cols = np.zeros((N_COLS, 64))
    cols[src >= 0] = det[ch][src[src >= 0]]
    t0 = time.perf_counter()
    a_dev = torch.from_numpy(np.concatenate([base, det[ch]])).cuda()
    b_dev = torch.from_numpy(cols).cuda().T.contiguous()
    pad = torch.from_numpy(src < 0).cuda()
    chunk = 2048
    g = torch.empty((chunk, N_COLS), dtype=torch.float32, device="cuda")
    n_bad = torch.zeros((), dtype=torch.int64, device="cuda")
    n_pad_bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for s0 in range(0, n_sel, chunk):
        n = min(chunk, n_sel - s0)
        ctx.debug_copy_gram_device(ch, s0, n, 0, N_COLS, g.data_ptr())
        ref = a_dev[s0:s0 + n] @ b_dev
        tol = ref.abs() * 2.0 ** -24 + 2.0 ** -45
        n_bad += ((g[:n].double() - ref).abs() > tol).sum()
        n_pad_bad += (g[:n][:, pad].view(torch.int32) != 0).sum()
    n_bad, n_pad_bad = int(n_bad), int(n_pad_bad)
    print(f"whole Gram table, channel {ch}: {time.perf_counter() - t0:.2f} s, {n_bad} entries out of tolerance")
    assert n_bad == 0
    assert n_pad_bad == 0                                              # every pad column exactly +0.0f


# ---- uploaded tiles -------------------------------------------------------------------------------------------------------
def test_uploaded_tiles_are_the_host_function_s(ia, ctx, dic):
    """byte for byte: pins the upload and the [channel][block] order of the detail tiles"""
    base, rows, det, off = dic
    want, _ = ia.api.filter_tiles(base, 32, 1)
    assert (ctx.debug_copy_filter_tiles(-1) == want).all()
    seen = {}
    for ch in range(3):
        for blk in (0, 1, 255, 509):
            want, _ = ia.api.filter_tiles(det[ch][off[blk]:off[blk] + rows[blk]], 4, 1)
            got = ctx.debug_copy_filter_tiles(ch, blk)
            assert (got == want).all(), (ch, blk)
            seen[ch, blk] = got.tobytes()
    # different answers, so that an offset cannot hide: the channels of every block, and blocks 0, 1, 255 of every channel (block 509
    # belongs to base row 509 = -row 0, the same segmentation as block 0)
    for blk in (0, 1, 255, 509):
        assert len({seen[ch, blk] for ch in range(3)}) == 3
    for ch in range(3):
        assert len({seen[ch, blk] for blk in (0, 1, 255)}) == 3


# ---- screen probe ------------------------------------------------------------------------------------------------------------
def probe(torch, ctx, ch, blk, vectors):
    v = torch.from_numpy(np.ascontiguousarray(vectors, np.float64)).cuda()
    n = v.shape[0]
    approx = torch.full((n, 576), SENTINEL, dtype=torch.float32, device="cuda")
    bound = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    ctx.debug_screen_probe_device(ch, blk, v.data_ptr(), n, approx.data_ptr(), bound.data_ptr())
    torch.cuda.synchronize()
    return approx.cpu().numpy(), bound.cpu().numpy()


@pytest.fixture(scope="module")
def base_exact(dic):
    """class name -> (vectors, exact projections on the 510 base rows), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            v = sc.residual_class(name, dic[0])
            cache[name] = (v, sc.exact_products(v, dic[0]))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sc.CLASSES)
def test_screen_probe_stays_inside_the_bound(torch, ctx, dic, base_exact, name):
    base, rows, det, off = dic
    v, exact_base = base_exact(name)
    want_bound = sc.reference_bound(v)
    worst = 0.0
    first = None
    for ch in range(3):
        for blk in (0, 1, 509):
            approx, bound = probe(torch, ctx, ch, blk, v)
            nr = int(rows[blk])
            exact_blk = sc.exact_products(v, det[ch][off[blk]:off[blk] + nr])
            ulp = np.spacing(want_bound.astype(np.float32)).astype(np.longdouble)
            assert (np.abs(bound.astype(np.longdouble) - want_bound) <= 2 * ulp).all(), (ch, blk)
            E = bound.astype(np.longdouble)[:, None]
            r_base = np.abs(approx[:, :509].astype(np.longdouble) - exact_base[:, :509]) / E
            r_blk = np.abs(approx[:, 512:512 + nr].astype(np.longdouble) - exact_blk) / E
            worst = max(worst, float(r_base.max()), float(r_blk.max()))
            assert (r_base <= 1).all() and (r_blk <= 1).all(), (ch, blk, float(r_base.max()), float(r_blk.max()))
            # no filter copy: base row 509 (ties with row 0 exactly), rows 510, 511, the block's pad rows
            assert (approx[:, 509:512] == 0).all() and (approx[:, 512 + nr:] == 0).all(), (ch, blk)
            assert (exact_base[:, 509] == -exact_base[:, 0]).all()
            if first is None:
                first = approx[:, :512].copy()
            else:
                assert (bits(approx[:, :512]) == bits(first)).all()    # the base rows do not depend on the block
            if name == "with_zero":
                assert (approx[sc.ZERO_SLOT] == 0).all() and bound[sc.ZERO_SLOT] == np.float32(sc.K_ABS)
    print(f"screen probe, class {name}: worst |approx - exact| / E_b = {worst:.3g}")


@pytest.mark.parametrize("name", ["gaussian", "magnitudes", "subnormal"])
def test_screen_probe_one_vector_equals_sixteen(torch, ctx, dic, name):
    v = sc.residual_class(name, dic[0])
    a16, b16 = probe(torch, ctx, 1, 509, v)
    for slot in (0, 15):
        a1, b1 = probe(torch, ctx, 1, 509, v[slot:slot + 1])
        assert (bits(a1[0]) == bits(a16[slot])).all() and bits(b1)[0] == bits(b16)[slot]
    a5, _ = probe(torch, ctx, 1, 509, v[:5])
    assert (bits(a5) == bits(a16[:5])).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ia, torch, ctx):
    A = ia.api.MPC_ERR_ARGUMENT
    n_sel = sc.NUM_BASE + 31622
    buf = torch.zeros(16 * 576, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()

    def refused(call):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == A
    for ch in (-1, 3):
        refused(lambda: ctx.debug_copy_gram_device(ch, 0, 1, 0, 1, p))
        refused(lambda: ctx.debug_screen_probe_device(ch, 0, p, 1, p, p))
    for ch in (-2, 3):
        refused(lambda: ctx.debug_copy_filter_tiles(ch, 0))
    for blk in (-1, 510):
        refused(lambda: ctx.debug_copy_filter_tiles(0, blk))
        refused(lambda: ctx.debug_screen_probe_device(0, blk, p, 1, p, p))
    for n in (0, 17, -1):
        refused(lambda: ctx.debug_screen_probe_device(0, 0, p, n, p, p))
    for rect in ((-1, 1, 0, 1), (0, 0, 0, 1), (n_sel, 1, 0, 1), (n_sel - 1, 2, 0, 1), (0, n_sel + 1, 0, 1), (0, 1, -1, 1), (0, 1, 0, 0),
                 (0, 1, N_COLS, 1), (0, 1, N_COLS - 1, 2), (0, 1, 1, N_COLS), (2 ** 31 - 1, 2 ** 31 - 1, 0, 1), (0, 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        refused(lambda: ctx.debug_copy_gram_device(0, *rect, p))
    refused(lambda: ctx.debug_copy_gram_device(0, 0, 1, 0, 1, 0))
    refused(lambda: ctx.debug_screen_probe_device(0, 0, 0, 1, p, p))
    refused(lambda: ctx.debug_screen_probe_device(0, 0, p, 1, 0, p))
    refused(lambda: ctx.debug_screen_probe_device(0, 0, p, 1, p, 0))
    refused(lambda: ctx.debug_screen_probe_device(0, 0, p + 8, 1, p, p))           # alignment of the vector loads
    L = ia.load_library()
    assert L.mpc_debug_copy_filter_tiles(ctx.h, 0, 0, None) == A
    for k in range(6):                                                             # each null pointer of the Gram kernel's entry
        args = [p] * 6
        args[k] = 0
        refused(lambda: ia.api.debug_gram_device(*args[:5], 3, 130, args[5]))
    refused(lambda: ia.api.debug_gram_device(p, p, p, p, p, 0, 130, p))
    refused(lambda: ia.api.debug_gram_device(p, p, p, p, p, 3, 2, p))
    assert not buf.any()                                                           # and nothing was written
    host = ia.create_compression_context(8, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        host.debug_screen_probe_device(0, 0, p, 1, p, p)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host.close()
    # the last valid rectangle and block are accepted
    assert gram_rect(torch, ctx, 2, n_sel - 1, 1, N_COLS - 64, 64).shape == (1, 64)
    assert ctx.debug_copy_filter_tiles(2, 509).any()
