"""Numpy model of the pursuit kernel's top-two key tracking (mp_pursuit.hip: TopKeys::see, TopKeys::see4, track_tile, pair_keys) and
the case classes of its tests (tests/test_track_keys_model.py on the CPU, tests/test_gpu_track_keys.py on the device).

A key is a value's float32 bit pattern with the sign and the low mantissa bits replaced by a code that names the row:
key = (bits & keep) | code.  see() is the definition: k2 = med3(k1, k2, key), k1 = max(k1, key).  The grouped form takes four keys at
once: m1 = max3(k1, a, b), s1 = med3(k1, a, b), m2 = max3(m1, c, d), s2 = med3(m1, c, d), k1 = m2, k2 = max3(k2, s1, s2).

Keys are compared here as unsigned integers.  The kernel takes the medians with v_med3_f32; for non-negative finite floats the two
orders are the same.  NaN and infinity bit patterns (exponent 255) are out of scope on purpose: a tile-channel whose residual norm
or pair bound is not below kHuge is diverted (`odd`, `oddp`) to the exhaustive evaluation before any key is read, so no result
depends on what the tracking does with them."""
import itertools

import numpy as np

KEEP_ROW = np.uint32(0x7FFFFF80)           # kKeepRow: 7 code bits, tile (5) and row within the lane's four (2)
KEEP_PAIR = np.uint32(0x7FFFFE00)          # kKeepPair: 9 code bits, pair (5), tile (2), row (2)
BASE_TILES, BLOCK_TILES = 32, 4
ROW_VALUES = 4 * (BASE_TILES + BLOCK_TILES)      # 144 per lane
LANES = 64
FLT_MAX_BITS = 0x7F7FFFFF


def u32(a):
    return np.asarray(a, dtype=np.uint32)


def med3(a, b, c):
    return np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))


def make_key(bits, keep, code):
    return (u32(bits) & keep) | u32(code)


def see(k1, k2, key):
    """TopKeys::see on keys: returns the new (k1, k2)."""
    return np.maximum(k1, key), med3(k1, k2, key)


def see4_sequential(k1, k2, keys):
    for key in keys:
        k1, k2 = see(k1, k2, key)
    return k1, k2


def see4_grouped(k1, k2, keys):
    a, b, c, d = keys
    m1 = np.maximum(np.maximum(k1, a), b)
    s1 = med3(k1, a, b)
    m2 = np.maximum(np.maximum(m1, c), d)
    s2 = med3(m1, c, d)
    return m2, np.maximum(np.maximum(k2, s1), s2)


def track_rows(bits, see4):
    """Pass 1 of one wave: bits[lanes, 144], [4 * tile + v]; tiles 0 .. 31 are the base tiles, 32 .. 35 DetailBasis[0], each with
    codes 4 * tile + v.  Returns base (k1, k2), block (k1, k2), each [lanes]."""
    bits = u32(bits)
    out = []
    for first, tiles in ((0, BASE_TILES), (BASE_TILES, BLOCK_TILES)):
        k1 = np.zeros(bits.shape[0], np.uint32)
        k2 = np.zeros(bits.shape[0], np.uint32)
        for t in range(tiles):
            keys = [make_key(bits[:, 4 * (first + t) + v], KEEP_ROW, 4 * t + v) for v in range(4)]
            k1, k2 = see4(k1, k2, keys)
        out += [k1, k2]
    return out


def track_pair(p_bits, bound, rows, pair, see4):
    """pair_keys of one pair: p_bits[lanes, 16], [4 * t + v] = P of row 16 t + 4 h + v (h = lane >> 4); keys of |P| + bound with
    codes pair << 4 | t << 2 | v, 0 for the pad rows 62 and 63 of a shorter block.  Returns k1, k2, bits of the largest |P|."""
    p = np.abs(u32(p_bits).view(np.float32))
    lanes = p.shape[0]
    h = np.arange(lanes) >> 4
    ub = (p + np.float32(bound)).astype(np.float32)
    ub[:, 14] = np.where((h == 3) & (rows < 63), np.float32(0), ub[:, 14])
    ub[:, 15] = np.where((h == 3) & (rows < 64), np.float32(0), ub[:, 15])
    ub_bits = ub.view(np.uint32)
    k1 = np.zeros(lanes, np.uint32)
    k2 = np.zeros(lanes, np.uint32)
    for t in range(4):
        keys = [make_key(ub_bits[:, 4 * t + v], KEEP_PAIR, (pair << 4) | (t << 2) | v) for v in range(4)]
        k1, k2 = see4(k1, k2, keys)
    return k1, k2, p.max(axis=1).view(np.uint32)


# ---- case classes ---------------------------------------------------------------------------------------------------
def finite_bits(rng, shape):
    """random float32 bit patterns, either sign, any exponent but 255 (zeros and subnormals included)"""
    b = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    exp255 = (b & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    return np.where(exp255, b & np.uint32(0xFF7FFFFF), b)


def orderings_of_six():
    """all 720 orders of six keys that stay distinct under both masks: [720, 6] bit patterns"""
    six = np.array([0x3F800000 + 0x1000 * i for i in (1, 2, 3, 5, 8, 13)], np.uint32)
    return np.array([six[list(p)] for p in itertools.permutations(range(6))], np.uint32)


def rows_with_every_ordering():
    """bits[64, 144] that put all 720 orderings in front of the tracking of a wave, state first: tile pair (2 j, 2 j + 1) of a lane
    holds one ordering as [p0, p1, 0, 0], [p2, p3, p4, p5], its values scaled by 2^(2 j) so that whatever the tiles before left in
    (k1, k2) lies below all six: the group of four meets the state top2(p0, p1).  18 orderings per lane (16 in the base tiles, 2 in the
    block tiles, whose tracking starts from zero), 1152 slots for 720 orderings (they wrap round)."""
    perms = orderings_of_six()
    bits = np.zeros((LANES, ROW_VALUES), np.uint32)
    n = 0
    for lane in range(LANES):
        for j in range(18):
            level = j if j < 16 else j - 16
            p = perms[n % len(perms)] + np.uint32(level << 24)      # exponent + 2 level
            n += 1
            bits[lane, 8 * j: 8 * j + 2] = p[:2]
            bits[lane, 8 * j + 4: 8 * j + 8] = p[2:]
    assert n >= len(perms)
    return bits


def pairs_with_orderings(first):
    """p_bits[64, 16]: lane l holds ordering first + l as [p0, p1, 0, 0], [p2 .. p5], zeros"""
    perms = orderings_of_six()
    bits = np.zeros((LANES, 16), np.uint32)
    for lane in range(LANES):
        p = perms[(first + lane) % len(perms)]
        bits[lane, 0:2] = p[:2]
        bits[lane, 4:8] = p[2:]
    return bits


def equal_before_code(rng, shape):
    """every group of four holds one value four times (either sign): only the codes tell the keys apart"""
    b = finite_bits(rng, shape[:-1] + (shape[-1] // 4, 1))
    b = np.broadcast_to(b, shape[:-1] + (shape[-1] // 4, 4)).reshape(shape).copy()
    sign = rng.integers(0, 2, size=shape, dtype=np.uint64).astype(np.uint32) << np.uint32(31)
    return b ^ sign


def device_cases(seed=20260001):
    """(name, row_bits[64, 144], pair_bits[64, 16], bound, rows, pair) for one probe launch each.  The pair bounds keep |P| + bound
    finite; 62-, 63- and 64-row blocks take the pad rule through its three outcomes."""
    rng = np.random.default_rng(seed)
    small = lambda shape: finite_bits(rng, shape) & np.uint32(0xBFFFFFFF)      # below 2: room for the bound
    top = np.full((LANES, ROW_VALUES), FLT_MAX_BITS, np.uint32)
    top[::2] ^= np.uint32(0x80000000)
    mixed = finite_bits(rng, (LANES, ROW_VALUES))
    mixed[rng.random((LANES, ROW_VALUES)) < 0.05] = FLT_MAX_BITS
    return [
        ("orderings", rows_with_every_ordering(), pairs_with_orderings(0), 0.0, 64, 0),
        ("orderings_pads", rows_with_every_ordering()[::-1].copy(), pairs_with_orderings(64), 0.0, 62, 31),
        ("random_62", finite_bits(rng, (LANES, ROW_VALUES)), small((LANES, 16)), 0.37, 62, 5),
        ("random_63", finite_bits(rng, (LANES, ROW_VALUES)), small((LANES, 16)), 1.0e-3, 63, 17),
        ("random_64", finite_bits(rng, (LANES, ROW_VALUES)), small((LANES, 16)), 3.0e-20, 64, 30),
        ("equal_62", equal_before_code(rng, (LANES, ROW_VALUES)), equal_before_code(rng, (LANES, 16)) & np.uint32(0xBFFFFFFF), 0.0, 62, 9),
        ("equal_63", equal_before_code(rng, (LANES, ROW_VALUES)), equal_before_code(rng, (LANES, 16)) & np.uint32(0xBFFFFFFF), 2.5, 63, 1),
        ("zeros_62", np.zeros((LANES, ROW_VALUES), np.uint32), np.zeros((LANES, 16), np.uint32), 0.0, 62, 0),
        ("zeros_64_bound", np.zeros((LANES, ROW_VALUES), np.uint32), np.zeros((LANES, 16), np.uint32), 0.125, 64, 31),
        ("flt_max", top, top[:, :16].copy(), 0.0, 63, 12),
        ("flt_max_mixed", mixed, mixed[:, :16].copy(), 0.0, 64, 3),
    ]
