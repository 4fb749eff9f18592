"""Hand-made records for stream assembly and its inverse, shared by the host test and the device test (nothing here needs a GPU, and
nothing here calls project code): the stage that turns per-tile records into the container's 6K symbol streams (mp_streams.hip: count,
scan, scatter, dc) and back (gather, window rank, crop).

A case is (W, H, K, counts[tiles, 3], words[tiles, 3, K], quant): tile t = tx * tiles_y + ty, a word = deltaId | intCoeff << 16.  The word at
(t, ch, i) is a function of (t, ch, i) that differs between neighbours in every direction, dead steps included (garbage behind a count:
nothing may carry it over), so a symbol written one place off changes the bytes.  The counts follow one PATTERN per channel, and the
three channels of a frame differ on purpose: the kernels keep per-channel state (wave_live, the DC `prev`) that a neighbour can leak
into.  Tile counts are the smallest that reach each branch: 1; 63 / 64 / 65 (a wave's edge); 1023 / 1024 / 1025 (a block's edge); 2049
(three blocks, a tail of one tile); 66 563 = 257 x 259 (66 blocks: the scan's second trip of 64), at K = 2 to stay small.

Two symbol families:
  wild   deltaId and coefficients over all of u16, 0, 1, 0x7FFF, 0x8000 and 0xFFFF forced in; step-0 coefficients in runs
         0, 0xFFFF, 0, 0x8000, 0x7FFF, ... so that the difference of neighbouring live tiles does not fit 16 bits.  The reference
         truncates there (CompressedImage.cpp:428-446, BitBuffer.h:116) and so must the device; such a container does not decode back
         to these records, which is why the round trips use the other family.  `narrow` cases stay within NARROW distinct values per
         half, the others do not (the device entropy stage and the host route).
  tame   any deltaId; step-0 coefficient symbols in 0 ... 0x7FFF, so neighbouring sums move by less than 2^15 and the container
         decodes back to the same records (include/mpcodec.h: the caveat of mpc_truncate_container).

The model: `streams` is CompressedImage.cpp:535-572 in numpy (per channel and step the live tiles' two halves, in tile order, the step-0
coefficients not differenced), `crop` the records of a tile rectangle.  Expected container bytes always come from the ORACLE's
writeCompressed of the model's streams (`container`, `crop_container`), never from project code.

`coded_streams` restates the same thing the way the kernels compute it -- a position is block offset + waves in front + rank inside
the wave, block offsets from an exclusive scan in trips of 64, the three step-0 coefficient streams differenced -- with a `mutant=`
switch for the mistakes these kernels can make.  It exists only to show that the cases tell right from wrong: no expected byte of
any test comes from it.  Notes on three of the mutants:
  no_clamp        a count above K is not clamped where the blocks are counted (the histogram has no bin for it), so the blocks behind
                  lose a position.  It needs a count above K, which only the case `above_k` has; no route is given that case but the
                  model and the crop.
  crop_keeps_dead, crop_y_outer   mistakes of the crop; the first shows only in the records (`crop`), since no container holds a dead
                  step."""
import functools

import numpy as np

SEED = 20261020
BLOCK, WAVE, TRIP = 1024, 64, 64
FORCED = (0, 1, 0x7FFF, 0x8000, 0xFFFF)
DC_RUN = (0, 0xFFFF, 0, 0x8000, 0x7FFF, 0xFFFF, 1, 0x8001)
NARROW = 199
MUTANTS = ("rank_per_wave", "no_block_offset", "inclusive_scan", "carry_lost", "stale_wave_live", "dc_prev_across", "dc_clamp",
           "swap_halves", "dc_ch0_only", "no_clamp")
CROP_MUTANTS = ("crop_keeps_dead", "crop_y_outer")

# name: (tiles_x, tiles_y, (pixels short of whole tiles: right, bottom), K, family, one pattern per channel)
CASES = {
    "t1": (1, 1, (3, 5), 1, "narrow", ("full", "empty", "full")),                        # a single tile
    "t63": (9, 7, (3, 5), 8, "wild", ("mod", ("lone", 62), "half")),                       # one tile short of a wave; the last tile alone
    "t64": (8, 8, (0, 0), 2, "narrow", (("lone", 63), ("pair", 0, 63), "full")),         # lane 63 alone; two step-0 tiles
    "t65": (13, 5, (0, 0), 5, "wild", (("lone", 64), ("lone", 0), "mod")),                 # lane 0 of wave 1 alone; tile 0 alone
    "t65_empty": (5, 13, (0, 0), 2, "tame", ("empty", "empty", "empty")),                 # no record at all
    "t1023": (33, 31, (0, 0), 8, "tame", ("waves", "waves_odd", "mod")),                  # waves alternately full and empty
    "t1024": (32, 32, (0, 0), 1, "wild", (("lone", 1023), "half", ("lone", 63))),          # lane 63 of wave 15 of block 0 alone
    "t1025": (25, 41, (0, 0), 32, "tame", ("mod", "half", ("lone", 1024))),                # tile 1024 alone: block 1 is one tile
    "t1025_gap": (41, 25, (0, 0), 8, "wild", ("full", "empty", "full")),                   # an empty channel between two full ones
    "t2049": (683, 3, (0, 0), 5, "tame", ("hole", "block1", "half")),                      # an empty block between live ones, and its inverse
    "t2049_lone": (3, 683, (0, 0), 5, "narrow", (("lone", 1024), ("lone", 2048), ("pair", 1023, 1024))),
    "t66563": (257, 259, (0, 0), 2, "tame", ("half", "blocks", "mod")),                   # 66 blocks; blocks alternately full and empty
}
# a count of K + 1 in block 0 of a frame of three blocks: for the model's no_clamp mutant and the crop alone
ABOVE_K = ("above_k", 683, 3, 5, 700)
BIG = "t66563"
WILD = tuple(n for n, c in CASES.items() if c[4] != "tame")
TAME = tuple(n for n, c in CASES.items() if c[4] == "tame")

# Rectangles of the tame frames in tiles, (tx0, tx1, ty0, ty1); t = tx * tiles_y + ty, so in t2049 t = 3 tx + ty, in t1025 t = 41 tx + ty.
# What each is for is its name; `check` below asserts it.
RECTS = {
    "t2049": {
        "first_64": (21, 31, 1, 3), "last_63": (10, 22, 0, 1), "first_63": (21, 40, 0, 3),
        "first_1024": (341, 400, 1, 3), "last_1023": (300, 342, 0, 1), "first_1023": (341, 345, 0, 3), "last_1024": (330, 342, 0, 2),
        "inside_block_1": (400, 500, 0, 3), "column": (341, 342, 0, 3), "last_tile": (682, 683, 2, 3), "last_columns": (600, 683, 0, 3),
    },
    "t1025": {"first_64": (1, 3, 23, 41), "last_1023": (23, 25, 38, 40), "last_tile": (24, 25, 40, 41), "column": (24, 25, 0, 41)},
}
EDGES = {"first_64": (64, None), "last_63": (None, 63), "first_63": (63, None), "first_1024": (1024, None), "last_1023": (None, 1023),
         "first_1023": (1023, None), "last_1024": (None, 1024)}
STEP_CUTS = {"t1025": (1, 31, 32), "t2049": (1, 4, 5)}        # 1, K - 1 and K


def _mix(t, ch, i, salt):
    """a u32 per (t, ch, i): a fixed integer hash, vectorised over t"""
    x = (np.asarray(t, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(ch * 0x85EBCA77 + i * 0xC2B2AE3D + salt * 0x27D4EB2F)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    return x.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _narrow_table():
    rng = np.random.default_rng(SEED)
    rest = rng.permutation(np.setdiff1d(np.arange(65536), FORCED))[:NARROW - len(FORCED)]
    return np.concatenate([FORCED, rest]).astype(np.int64)


def make_words(tiles, K, family, salt):
    t = np.arange(tiles)
    words = np.zeros((tiles, 3, K), np.uint32)
    forced = np.array(FORCED, np.int64)
    for ch in range(3):
        for i in range(K):
            h = _mix(t, ch, i, salt)
            if family == "narrow":
                table = _narrow_table()
                low, high = table[(t + 3 * ch + 5 * i) % NARROW], table[(h >> 16) % (NARROW - 2)]
            else:
                low, high = h & 0xFFFF, h >> 16
                if family == "wild":                            # the forced values, each about one symbol in sixty
                    sel, sel2 = (h >> 8) % 61, (h >> 3) % 59
                    low = np.where(sel < 5, forced[sel % 5], low)
                    high = np.where(sel2 < 5, forced[sel2 % 5], high)
            if i == 0:
                if family == "tame":
                    high = high & 0x7FFF
                else:                                           # runs that wrap, sixteen tiles at a time, between stretches of anything
                    high = np.where((t // 16) % 2 == 0, np.array(DC_RUN, np.int64)[(t + ch) % len(DC_RUN)], high)
            words[:, ch, i] = (low | (high << 16)).astype(np.uint32)
    return words


def make_counts(pattern, tiles, K, rng):
    t = np.arange(tiles)
    if isinstance(pattern, tuple):                              # ("lone", t) / ("pair", t, t'): these tiles at K, nothing else
        assert pattern[0] in ("lone", "pair") and len(pattern) == (2 if pattern[0] == "lone" else 3)
        return np.where(np.isin(t, pattern[1:]), K, 0)
    if pattern == "full":
        return np.full(tiles, K)
    if pattern == "empty":
        return np.zeros(tiles, np.int64)
    if pattern == "mod":
        return t % (K + 1)
    if pattern == "waves":
        return np.where((t // WAVE) % 2 == 0, K, 0)
    if pattern == "waves_odd":
        return np.where((t // WAVE) % 2 == 1, K, 0)
    if pattern == "blocks":
        return np.where((t // BLOCK) % 2 == 0, K, 0)
    if pattern == "block1":
        return np.where(t // BLOCK == 1, K, 0)
    if pattern == "hole":                                       # block 1 empty, every depth 1 ... K on either side of it
        return np.where(t // BLOCK == 1, 0, 1 + t % K)
    if pattern == "half":                                       # random, half the tiles dead
        return np.where(rng.random(tiles) < 0.5, 0, rng.integers(1, K + 1, tiles))
    raise ValueError(pattern)


def tables(K):
    """the header's steps [3, K] (u16): nothing here depends on them but the header's bytes"""
    return (np.arange(1, 3 * K + 1).reshape(3, K) * 3).astype(np.uint16)


class Case:
    def __init__(self, name, tiles_x, tiles_y, short, K, family, patterns, counts, words):
        self.name, self.tiles_x, self.tiles_y, self.K, self.family, self.patterns = name, tiles_x, tiles_y, K, family, patterns
        self.W, self.H = 8 * tiles_x - short[0], 8 * tiles_y - short[1]
        self.tiles = tiles_x * tiles_y
        self.counts, self.words, self.quant = counts, words, tables(K)
        self.counts.setflags(write=False)
        self.words.setflags(write=False)

    def rect_pixels(self, grid):
        tx0, tx1, ty0, ty1 = grid
        return 8 * tx0, 8 * ty0, min(8 * tx1, self.W) - 8 * tx0, min(8 * ty1, self.H) - 8 * ty0

    def tile_range(self, grid):
        """(first tile, last tile) of a rectangle"""
        tx0, tx1, ty0, ty1 = grid
        return tx0 * self.tiles_y + ty0, (tx1 - 1) * self.tiles_y + ty1 - 1


@functools.lru_cache(maxsize=None)
def case(name):
    if name == ABOVE_K[0]:
        _, tiles_x, tiles_y, K, at = ABOVE_K
        base = case("t2049")
        counts = np.array(base.counts)
        counts[:, 0] = np.where(np.arange(base.tiles) // BLOCK == 1, 0, K)
        counts[at, 0] = K + 1
        return Case(name, tiles_x, tiles_y, (0, 0), K, "tame", ("full but block 1", "block1", "half"), counts, np.array(base.words))
    tiles_x, tiles_y, short, K, family, patterns = CASES[name]
    salt = sorted(CASES).index(name)
    rng = np.random.default_rng([SEED, salt])
    tiles = tiles_x * tiles_y
    counts = np.stack([make_counts(p, tiles, K, rng) for p in patterns], axis=1).astype(np.uint16)
    return Case(name, tiles_x, tiles_y, short, K, family, patterns, counts, make_words(tiles, K, family, salt))


# ---- the model --------------------------------------------------------------------------------------------------------------------

def streams(counts, words, K):
    """the 6K streams as the encoder holds them (CompressedImage.cpp:535-572): codes[2K*ch + 2i] = deltaId, [+ 1] = intCoeff of every
    tile with count > i, tiles in the order given; step-0 coefficients not differenced"""
    c = np.asarray(counts, np.int64)
    out = []
    for ch in range(3):
        for i in range(K):
            w = np.asarray(words)[c[:, ch] > i, ch, i]
            out += [(w & 0xFFFF).astype(np.uint16), (w >> 16).astype(np.uint16)]
    return out


def crop(counts, words, tiles_x, tiles_y, rect_tiles, steps, mutant=None):
    """the records of the tile rectangle (tx0, tx1, ty0, ty1) as a frame of their own: tile (tx - tx0) * nty + (ty - ty0) takes tile
    tx * tiles_y + ty; counts min(count, K, steps), the steps behind them zero"""
    assert mutant is None or mutant in CROP_MUTANTS
    tx0, tx1, ty0, ty1 = rect_tiles
    assert 0 <= tx0 < tx1 <= tiles_x and 0 <= ty0 < ty1 <= tiles_y and steps >= 1
    K = words.shape[2]
    source = np.arange(tx0, tx1)[:, None] * tiles_y + np.arange(ty0, ty1)[None, :]
    source = (source.T if mutant == "crop_y_outer" else source).reshape(-1)
    c = np.minimum(np.minimum(np.asarray(counts, np.int64)[source], K), steps)
    live = np.arange(K)[None, None, :] < c[:, :, None]
    kept = words[source] if mutant == "crop_keeps_dead" else np.where(live, words[source], 0)
    return c.astype(np.uint16), kept.astype(np.uint32)


def zigzag(d):
    d = np.asarray(d, np.int64)
    return (d << 1) ^ (d >> 63)


def unzigzag(z):
    z = np.asarray(z, np.int64)
    return (z >> 1) ^ -(z & 1)


def dc_difference(v, first_prev=0, clamp=False):
    """CompressedImage.cpp:428-446: zigzagEncode(v - prev) in 32 bits, stored in 16.  clamp: the mutant that saturates instead"""
    v = np.asarray(v, np.int64)
    d = v - np.concatenate([[first_prev], v[:-1]])[:v.size]
    if clamp:
        d = np.clip(d, -32768, 32767)
    return (zigzag(d) & 0xFFFF).astype(np.uint16)


def dc_read_back(coded):
    """CompressedImage.cpp:690-705: what a reader makes of a differenced stream: the running sum of zigzagDecode, stored in 16 bits"""
    return (np.cumsum(unzigzag(coded)) & 0xFFFF).astype(np.uint16)


def read_back(held, K):
    """the streams a reader returns for a container written from `held`: the same, but for the step-0 coefficient streams where a
    difference did not fit 16 bits"""
    out = list(held)
    for ch in range(3):
        out[2 * K * ch + 1] = dc_read_back(dc_difference(held[2 * K * ch + 1]))
    return out


def coded_streams(counts, words, K, mutant=None):
    """the 6K streams as the device hands them to the entropy stage (step-0 coefficient streams differenced), computed the kernels'
    way: position = block offset + live tiles of the waves in front + rank inside the wave.  mutant: one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS
    c = np.asarray(counts, np.int64)
    tiles = c.shape[0]
    t = np.arange(tiles)
    blocks = -(-tiles // BLOCK)
    block, wave = t // BLOCK, t // WAVE                          # wave: numbered through the frame, 16 to a block
    fronts, held = {}, []
    for ch in range(3):
        for i in range(K):
            live = c[:, ch] > i
            counted = live & (c[:, ch] <= K) if mutant == "no_clamp" else live
            per_block = np.bincount(block[counted], minlength=blocks)
            incl = np.cumsum(per_block)
            if mutant == "carry_lost":                          # every trip of 64 blocks starts from nothing
                incl = incl - np.repeat(np.concatenate([[0], incl[TRIP - 1::TRIP]]), TRIP)[:blocks]
            off = incl if mutant == "inclusive_scan" else incl - per_block
            if mutant == "no_block_offset":
                off = np.zeros_like(off)
            per_wave = np.bincount(wave[live], minlength=blocks * (BLOCK // WAVE)).reshape(blocks, BLOCK // WAVE)
            fronts[ch, i] = front = (np.cumsum(per_wave, axis=1) - per_wave).reshape(-1)
            if mutant == "stale_wave_live" and ch > 0:
                front = fronts[ch - 1, i]
            if mutant == "rank_per_wave":
                front = np.zeros_like(front)
            before = np.cumsum(live) - live                     # live tiles in front, in the whole frame
            rank = before - before[wave * WAVE]                 # ... in front inside the wave
            pos = (off[block] + front[wave] + rank)[live]
            size = int(per_block.sum())
            w = np.asarray(words)[live, ch, i].astype(np.int64)
            low, high = (w >> 16, w & 0xFFFF) if mutant == "swap_halves" else (w & 0xFFFF, w >> 16)
            for half in (low, high):
                s = np.zeros(size + tiles + 1, np.uint16)        # a wrong position lands somewhere; what is behind the size is lost
                s[pos] = half
                held.append(s[:size])
    coded = list(held)
    prev = 0
    for ch in range(3):
        v = held[2 * K * ch + 1]
        if not (mutant == "dc_ch0_only" and ch > 0):
            coded[2 * K * ch + 1] = dc_difference(v, prev if mutant == "dc_prev_across" else 0, clamp=mutant == "dc_clamp")
        if v.size:
            prev = int(v[-1])
    return coded


def code(held, K):
    """held streams -> as the entropy stage takes them"""
    out = list(held)
    for ch in range(3):
        out[2 * K * ch + 1] = dc_difference(held[2 * K * ch + 1])
    return out


# ---- expected bytes: the oracle's ---------------------------------------------------------------------------------------------------

_containers = {}


def oracle_bytes(oracle, W, H, K, quant, counts, words):
    return oracle.write_compressed(dict(W=W, H=H, K=K, bs=8, quant=quant, lengths=np.asarray(counts, np.uint16).reshape(-1),
                                        codes=streams(counts, words, K)))


def container(oracle, name):
    """the oracle's writeCompressed of the model's streams of a case, computed once"""
    if name not in _containers:
        c = case(name)
        _containers[name] = oracle_bytes(oracle, c.W, c.H, c.K, c.quant, c.counts, c.words)
    return _containers[name]


def crop_container(oracle, name, grid, steps):
    """the oracle's writeCompressed of the model's crop of a case; grid None = the whole frame"""
    c = case(name)
    grid = grid or (0, c.tiles_x, 0, c.tiles_y)
    if (name, grid, steps) not in _containers:
        counts, words = crop(c.counts, c.words, c.tiles_x, c.tiles_y, grid, steps)
        _, _, w, h = c.rect_pixels(grid)
        _containers[name, grid, steps] = oracle_bytes(oracle, w, h, c.K, c.quant, counts, words)
    return _containers[name, grid, steps]


# ---- what each case is for ----------------------------------------------------------------------------------------------------------

def _live_runs(c, ch):
    """the step-0 coefficient symbols of the live tiles of a channel, in tile order"""
    return (c.words[c.counts[:, ch] > 0, ch, 0] >> 16).astype(np.int64)


def check(name):
    """conditions on the inputs; the seed was chosen so that they hold"""
    c = case(name)
    K, tiles = c.K, c.tiles
    assert c.counts.shape == (tiles, 3) and c.words.shape == (tiles, 3, K) and c.counts.max(initial=0) <= K
    assert 1 <= K <= 32 and c.tiles_x == -(-c.W // 8) and c.tiles_y == -(-c.H // 8)
    # neighbours differ: along the tiles, the channels and the steps, dead steps included
    assert (c.words[1:] != c.words[:-1]).all() and (c.words[:, 1:] != c.words[:, :-1]).all() and (c.words[:, :, 1:] != c.words[:, :, :-1]).all()
    assert all(c.patterns[ch] != c.patterns[ch + 1] for ch in range(2)) or name == "t65_empty"      # a channel never repeats the one in front
    for ch, p in enumerate(c.patterns):
        col = c.counts[:, ch].astype(np.int64)
        live = np.flatnonzero(col)
        if isinstance(p, tuple):
            assert live.tolist() == sorted(p[1:]) and (col[live] == K).all() and max(p[1:]) < tiles
        elif p == "hole":
            assert tiles > 2 * BLOCK and not col[BLOCK:2 * BLOCK].any() and col[:BLOCK].all() and col[2 * BLOCK:].all()
            assert set(col[:BLOCK]) == set(range(1, K + 1))
        elif p == "block1":
            assert tiles > 2 * BLOCK and (col[BLOCK:2 * BLOCK] == K).all() and not col[:BLOCK].any() and not col[2 * BLOCK:].any()
        elif p == "blocks":
            assert tiles > 64 * BLOCK and all((col[b * BLOCK:(b + 1) * BLOCK] == (K if b % 2 == 0 else 0)).all() for b in range(-(-tiles // BLOCK)))
        elif p in ("waves", "waves_odd"):
            assert tiles > 2 * WAVE and all((col[w * WAVE:(w + 1) * WAVE] == (K if w % 2 == (p == "waves_odd") else 0)).all()
                                            for w in range(-(-tiles // WAVE)))
        elif p == "half":
            assert tiles < 8 or (0.35 < (col == 0).mean() < 0.65 and (tiles < 200 or set(col) == set(range(K + 1))))
        elif p == "mod":
            assert (col == np.arange(tiles) % (K + 1)).all()
        else:
            assert (col == {"full": K, "empty": 0}[p]).all()
    if name == "t1024":                                         # the lone tile is lane 63 of wave 15 of block 0
        (t,) = np.flatnonzero(c.counts[:, 0])
        assert (t // BLOCK, (t % BLOCK) // WAVE, t % WAVE) == (0, 15, 63) and c.counts[63, 2] == K
    if name == "t1025_gap":
        assert (c.counts[:, 0] == K).all() and not c.counts[:, 1].any() and (c.counts[:, 2] == K).all()
    if name == BIG:
        assert -(-tiles // BLOCK) > TRIP and all(c.counts[TRIP * BLOCK:, ch].any() for ch in range(3))
    runs = [_live_runs(c, ch) for ch in range(3)]
    if c.family == "tame":
        assert all((r <= 0x7FFF).all() for r in runs)
        assert all((np.abs(np.diff(np.concatenate([[0], r]))) < 2 ** 15).all() for r in runs)
    else:
        live = [c.words[c.counts[:, ch] > i, ch, i] for ch in range(3) for i in range(K)]
        symbols = np.concatenate(live) if live else np.zeros(0, np.uint32)
        if symbols.size >= 64:
            assert (symbols & 0xFFFF).max() >= 0x8000 and (symbols >> 16).max() >= 0x8000
        if any(r.size >= 16 for r in runs):                     # a difference that does not fit: the truncation is reached
            assert any((zigzag(np.diff(np.concatenate([[0], r]))) > 0xFFFF).any() for r in runs)
        distinct = max(len(np.unique(s)) for w in live for s in (w & 0xFFFF, w >> 16))
        longest = max(w.size for w in live)
        assert distinct <= NARROW if c.family == "narrow" else (longest < 1000 or distinct > 3 * NARROW)
    for what, grid in RECTS.get(name, {}).items():
        first, last = c.tile_range(grid)
        want = EDGES.get(what)
        assert want is None or (want[0] in (None, first) and want[1] in (None, last)), (name, what, first, last)
        if what == "inside_block_1":
            assert BLOCK <= first and last < 2 * BLOCK
        if what == "column":
            assert grid[1] - grid[0] == 1 and (grid[2], grid[3]) == (0, c.tiles_y)
        if what in ("last_tile", "last_columns"):
            assert last == tiles - 1 and (first == last) == (what == "last_tile")


def check_families():
    """over the wild cases together: every forced value in both halves, one and two live step-0 tiles in a channel, narrow and not"""
    low, high, live0 = set(), set(), set()
    for name in WILD:
        c = case(name)
        for ch in range(3):
            live0.add(int((c.counts[:, ch] > 0).sum()))
            for i in range(c.K):
                w = c.words[c.counts[:, ch] > i, ch, i]
                low |= set((w & 0xFFFF).tolist()) & set(FORCED)
                high |= set((w >> 16).tolist()) & set(FORCED)
    assert low == set(FORCED) and high == set(FORCED) and {0, 1, 2} <= live0
    assert {case(n).family for n in WILD} == {"wild", "narrow"}
    assert {case(n).K for n in CASES if case(n).tiles < 2049} >= {1, 2, 5, 8, 32}
    assert case("t2049").K == 5 and case("t2049_lone").K == 5 and case("t1025").K == 32 and case(BIG).K == 2
    assert sorted({case(n).tiles for n in CASES}) == [1, 63, 64, 65, 1023, 1024, 1025, 2049, 66563]
