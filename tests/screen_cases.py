"""Inputs of the screen-table tests (test_screen_cases.py on the CPU, test_gpu_screen_tables.py on the device), fixed seeds.

The pursuit kernel screens with three things that decide nothing by themselves, so that no record can show them wrong: the Gram
table (mp_gram_kernel), the split-bf16 filter tiles (filter_tiles, k order 1) and the bound E_b = 2^-13 |r~| + 2^-100 on
|MFMA approximation - exact projection|.  Here: the residual classes the bound is probed with, a small synthetic
dictionary that reaches the Gram kernel's shadow / pad-row / partial-tile branches, the sample of the resident table, and plain
numpy restatements (bf16 rounding, the operand layout as DESIGN.md 3 words it, the screen's arithmetic) to hold the product to."""
import numpy as np

NUM_BASE = 510
TILE_HALVES = 2048                 # 16-bit elements of a filter tile: 16 rows x 64 pixels x (hi, lo)
K_SLACK = 2.0 ** -13               # E_b = K_SLACK * |r~| + K_ABS
K_ABS = 2.0 ** -100
POS = (0, 1, 3, 2)                 # lane row h holds pixels 16 * POS[h] .. + 15 ("Layout")
CLASSES = ("gaussian", "pixels", "huge_projection", "magnitudes", "bf16_midpoints", "subnormal", "near_huge", "constant", "with_zero")
ZERO_SLOT = 5                      # the all-zero vector of class "with_zero"


def row_offsets(block_rows):
    """first detail row of every block (and the total as the last entry)"""
    return np.concatenate([[0], np.cumsum(np.asarray(block_rows, np.int64))])


# ---- residual classes: name -> float64 [16, 64] -------------------------------------------------
def residual_class(name, base):
    """`base`: the dictionary's base rows (class huge_projection takes 16 of them)."""
    rng = np.random.default_rng(7000 + CLASSES.index(name))
    if name == "gaussian":
        return 100.0 * rng.standard_normal((16, 64))
    if name == "pixels":                                   # centred 8-bit pixels
        return rng.integers(0, 256, (16, 64)).astype(np.float64) - 128.0
    if name == "huge_projection":                          # one huge projection among tiny ones
        rows = rng.choice(np.arange(1, base.shape[0]), size=16, replace=False)
        return 1000.0 * base[rows] + 1e-3 * rng.standard_normal((16, 64))
    if name == "magnitudes":                               # per-element magnitudes 10^U(-6, 6)
        return rng.choice([-1.0, 1.0], (16, 64)) * 10.0 ** rng.uniform(-6.0, 6.0, (16, 64))
    if name == "bf16_midpoints":                           # f32 values exactly between two bf16 values: hi rounds to even, lo = -+2^(e-8)
        return rng.choice([-1.0, 1.0], (16, 64)) * (1.0 + 2.0 ** -8) * 2.0 ** rng.integers(-12, 13, (16, 64)).astype(np.float64)
    if name == "subnormal":                                # f32 subnormals; the 2^-100 term of the bound rules
        return 1e-38 * rng.standard_normal((16, 64))
    if name == "near_huge":                                # |r~| about 8e28, just under the 1e30 beyond which the screen is skipped
        return 1e28 * rng.standard_normal((16, 64))
    if name == "constant":                                 # constant tiles
        return np.repeat(rng.choice([-1.0, 1.0], 16) * 10.0 ** rng.uniform(-2.0, 3.0, 16), 64).reshape(16, 64)
    if name == "with_zero":                                # one all-zero vector among the others
        v = 50.0 * rng.standard_normal((16, 64))
        v[ZERO_SLOT] = 0.0
        return v
    raise KeyError(name)


# ---- the small synthetic dictionary of the Gram kernel's own test ----------------------------------
SYN_NUM_BASE = 3
SYN_BLOCK_ROWS = (64, 62, 1)       # no pad row, two pad rows, 63 pad rows
SYN_N_SEL = SYN_NUM_BASE + sum(SYN_BLOCK_ROWS)      # 130: two full selector tiles and one of 2 rows
SYN_DUPLICATE = (0, 40, 7)         # block 0: row 40 = row 7
SYN_NEGATED = (1, 30, 3)           # block 1: row 30 = -row 3


def synthetic_dictionary():
    """-> base[3,64], detail[127,64] (random unit rows), block_rows[3], block_row_off[3], shadow[127] (the two planted rows)"""
    rng = np.random.default_rng(4242)
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1))[:, None]
    base = unit(rng.standard_normal((SYN_NUM_BASE, 64)))
    detail = unit(rng.standard_normal((sum(SYN_BLOCK_ROWS), 64)))
    off = row_offsets(SYN_BLOCK_ROWS)
    shadow = np.zeros(detail.shape[0], np.uint8)
    b, j, i = SYN_DUPLICATE
    detail[off[b] + j] = detail[off[b] + i]
    shadow[off[b] + j] = 1
    b, j, i = SYN_NEGATED
    detail[off[b] + j] = -detail[off[b] + i]
    shadow[off[b] + j] = 1
    return base, detail, np.asarray(SYN_BLOCK_ROWS, np.int32), off[:-1].astype(np.int32), shadow


# ---- the sample of the resident table ---------------------------------------------------------------
def sample_selector_tiles(n_sel):
    """tiles of 64 selectors: the first; the one holding sel 448 .. 511 (base row 509 and the base / detail boundary at 510); the
    last (4 rows of the real dictionary); eight seeded random ones"""
    last = (n_sel - 1) // 64
    rng = np.random.default_rng(911)
    others = rng.choice(np.setdiff1d(np.arange(1, last), [7]), size=8, replace=False)
    return [0, 7, last] + sorted(int(t) for t in others)


def sample_blocks():
    """blocks 0 (63 rows), 1 (62), 509 (63), 255 and four seeded random ones"""
    rng = np.random.default_rng(912)
    others = rng.choice(np.setdiff1d(np.arange(2, 509), [255]), size=4, replace=False)
    return [0, 1, 509, 255] + sorted(int(b) for b in others)


def selector_rows(base, detail_ch, sel_begin, sel_end):
    """rows sel_begin .. sel_end - 1 of a channel's Gram table as the pursuit's `resolve` reads a selector: sel < num_base is base
    row sel, otherwise detail row sel - num_base of the channel"""
    nb = base.shape[0]
    return np.array([base[s] if s < nb else detail_ch[s - nb] for s in range(sel_begin, sel_end)])


def block_columns(detail_ch, block_rows, blk):
    """the 64 columns 64 * blk + row of a channel's Gram table: detail row block_row_off[blk] + row, zero rows for the pads"""
    off = row_offsets(block_rows)
    cols = np.zeros((64, 64))
    cols[:block_rows[blk]] = detail_ch[off[blk]:off[blk] + block_rows[blk]]
    return cols


def exact_products(a, b):
    """a[m,64] . b[n,64]^T in long double -> longdouble [m, n]"""
    return np.asarray(a, np.longdouble) @ np.asarray(b, np.longdouble).T


def gram_violations(g, ref, abs_term=2.0 ** -46):
    """entries of the float32 g with |g - ref| > 2^-24 |ref| + abs_term: the one float rounding DESIGN.md 3 assumes of G, and 64
    double fmas on unit rows (64 * 2^-53) with a factor 2"""
    ref = np.asarray(ref, np.longdouble)
    err = np.abs(np.asarray(g, np.longdouble) - ref)
    return err > np.longdouble(2.0 ** -24) * np.abs(ref) + np.longdouble(abs_term)


# ---- bfloat16, restated from its definition ------------------------------------------------------------
def bf16_rne(x32):
    """float32 array -> uint16 bits of the nearest bfloat16, ties to the even significand.  From the definition: the two bfloat16
    neighbours of x (its 16 upper bits, and one step of the 8-bit significand further from zero), the nearer one in exact
    arithmetic, the one with an even last bit at equal distance.  (Finite inputs below the largest bfloat16.)"""
    x32 = np.ascontiguousarray(x32, np.float32)
    bits = x32.view(np.uint32)
    down = bits & np.uint32(0xFFFF0000)
    up = down + np.uint32(0x10000)
    xd = x32.astype(np.float64)
    d_down = np.abs(xd - down.view(np.float32).astype(np.float64))
    d_up = np.abs(up.view(np.float32).astype(np.float64) - xd)
    take_up = (d_up < d_down) | ((d_up == d_down) & (((down >> np.uint32(16)) & np.uint32(1)) == 1))
    return (np.where(take_up, up, down) >> np.uint32(16)).astype(np.uint16)


def bf16_value(h):
    """uint16 bits -> float32 values"""
    return (np.asarray(h, np.uint32) << np.uint32(16)).astype(np.uint32).view(np.float32)


def split_bf16(x):
    """float64 array -> (hi, lo) uint16 bits: hi = bf16(float32(x)), lo = bf16(float32(x) - hi)"""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    hi = bf16_rne(x32)
    lo = bf16_rne(x32 - bf16_value(hi))           # the difference is exact in float32
    return hi, lo


# ---- the operand layout, from DESIGN.md 3 ----------------------------------------------------------------
def operand_pixels(k_order):
    """pix[kk, lane, j]: the pixel that element j of lane `lane`'s 16-byte operand of MFMA kk (0, 1) holds.  k order 1 (the pursuit
    kernel): lane (row & 15, h) holds pixels 16 pos(h) .. + 15, the first eight in kk = 0, the next eight in kk = 1.  k order 0
    (the instruction's own: lane row h holds k = 8 h .. 8 h + 7 of each block of 32): pixel 32 kk + 8 h + j."""
    pix = np.zeros((2, 64, 8), np.int64)
    for kk in range(2):
        for lane in range(64):
            h = lane >> 4
            for j in range(8):
                pix[kk, lane, j] = 16 * POS[h] + 8 * kk + j if k_order == 1 else 32 * kk + 8 * h + j
    return pix


def decode_tiles(out, tiles, k_order):
    """uint16 [tiles * 2048] in operand order -> (hi, lo) uint16 [16 * tiles, 64] by (row, pixel): tile t is four operands of 64
    lanes x 8 elements, (kk = 0: hi, lo), (kk = 1: hi, lo); lane l of tile t belongs to row 16 t + (l & 15)"""
    t = np.asarray(out, np.uint16).reshape(tiles, 2, 2, 64, 8)         # tile, kk, part, lane, j
    pix = operand_pixels(k_order)
    hi = np.zeros((16 * tiles, 64), np.uint16)
    lo = np.zeros((16 * tiles, 64), np.uint16)
    seen = np.zeros((16 * tiles, 64), np.int64)
    for tile in range(tiles):
        for kk in range(2):
            for lane in range(64):
                row = 16 * tile + (lane & 15)
                hi[row, pix[kk, lane]] = t[tile, kk, 0, lane]
                lo[row, pix[kk, lane]] = t[tile, kk, 1, lane]
                seen[row, pix[kk, lane]] += 1
    assert (seen == 1).all()                     # the layout names every (row, pixel) exactly once
    return hi, lo


# ---- the screen's arithmetic as a numpy model ----------------------------------------------------------------
def model_bound(vectors):
    """E_b of each vector as the kernel computes it -> float32 [n]"""
    x = np.asarray(vectors, np.float64).astype(np.float32).astype(np.float64)
    rnorm = np.sqrt((x * x).sum(axis=1)).astype(np.float32) * np.float32(1.0000002)
    return np.float32(K_SLACK) * rnorm + np.float32(K_ABS)


def reference_bound(vectors):
    """2^-13 float32(|float32(r)|_2 * 1.0000002) + 2^-100 in long double -> longdouble [n] (the probe's is held to 2 ulp of this)"""
    x = np.asarray(vectors, np.float64).astype(np.float32).astype(np.longdouble)
    rnorm = (np.sqrt((x * x).sum(axis=1)) * np.longdouble(1.0000002)).astype(np.float32).astype(np.longdouble)
    return np.longdouble(K_SLACK) * rnorm + np.longdouble(K_ABS)


def model_screen(rows, vectors):
    """The screen's approximation of <row, vector> for rows[m,64] x vectors[n,64] -> float32 [n, m]: both operands split into
    hi / lo bf16, per kk the product groups hi.hi, hi.lo, lo.hi over the 32 pixels of that kk in k order 1, every product exact
    in float32, the 192 of them added one after the other in float32.  (The matrix core's own order inside an instruction is
    not documented: the model is a fair member of the family the bound covers, not a bit-exact twin.)"""
    ah, al = (bf16_value(p) for p in split_bf16(rows))
    bh, bl = (bf16_value(p) for p in split_bf16(vectors))
    pix = operand_pixels(1)
    terms = []
    for kk in range(2):
        order = pix[kk].reshape(4, 16, 8)[:, 0, :].reshape(-1)         # lane rows h = 0 .. 3 of slot 0: 32 pixels
        for a, b in ((ah, bh), (ah, bl), (al, bh)):
            terms.append(a[None, :, order] * b[:, None, order])        # float32, exact: 8-bit x 8-bit significands
    seq = np.concatenate(terms, axis=2)                                # [n, m, 192]
    return np.cumsum(seq, axis=2, dtype=np.float32)[:, :, -1]
