"""Inputs and host models of the pair-drift tests (test_pair_drift_cases.py on the CPU, test_gpu_pair_drift.py on the device).

The persistent pursuit kernel does not recompute the projections onto the rows of an unlocked detail block other than
DetailBasis[0] (a "pair": a tile-channel and such a block).  It keeps 64 float approximations P_b per pair in scratch memory, makes
them once with the screen's MFMAs from the residual that follows the unlocking step, and after every later step with atom a and
coefficient c updates them: P_b = fmaf(-float(c), G[a][b], P_b) with G the Gram table.  A bound E per pair, started as the MFMA
bound and grown by E = (E + 2^-21 (|float(c)| + |r~|)) * 1.000001f per update, is part of the survivor test, which is right only
while the exactly evaluated projection lies within |P_b| +- E.  No record shows a wrong P_b unless the true winner sits in the
pair and its P_b came out too low, so the tests read the scratch itself (mpc_debug_pair_scratch).

GROUPS of 16 vectors, one wave's slots (pair_round_cases.py): its `ramp`, `deep`, `mixed` and `one`; `with_row0`, whose vectors
contain base row 0, so that DetailBasis[0] is unlocked and its rows are chosen while pairs are held; and `deep` times 2^40 and
2^-40 (exact scalings: the vectors stay f32-valued and the quantiser scales with them).

STOP DEPTH.  Every group runs in the tiny-quant form (one step far below the data for all K steps) with 1e30 at index d: the
quantised coefficient of step d is 0, so the pursuit ends there, the oracle's returned residual is r_d (the residual entering the
ending step), and that is the residual the kept approximations stand for: the update of an ended slot is skipped, and a pair
created at step k gets its MFMA start from r_{k+1}.  The K cap is never used as an end (there the oracle's residual is one update
further on than the scratch).  The steps before d do not depend on d, so one replay per vector serves every depth.

REPLAY.  `replay` repeats the pursuit on the host from the chosen dictionary indices alone, in the flavour's own arithmetic: the
projection is the reference's chain (j ascending, product and sum rounded separately: float64 for the double flavour, float32 on
the rows rounded to float for the float flavour), q = round(p / step) half away from zero, c = step * q, r -= c * row with two
roundings.  Coefficients cannot be read back from the records: q is about 10^6 in the tiny form and the record keeps 16 bits of
its zig-zag.  The dictionary's index space grows by a block's rows at EVERY choice of a base row, a repeated one included; only
the first unlock of a block other than 0 makes a pair.  test_pair_drift_cases.py holds the replay to the oracle: the low 16 bits
of the zig-zag of its q are the oracle's intCoeff and its residual at the end is the oracle's, bit for bit.

Every pair block has 62 rows: the only blocks of 63 rows are 0, which is never a pair, and 509, which is never unlocked (base row
509 is -row 0 and loses the tie to it).  So the pad rows are always rows 62 and 63 (asserted in test_pair_drift_cases.py); there
is no 63-row case to make."""
from fractions import Fraction

import numpy as np

import pair_round_cases as prc
import pursuit_cases as pc
import screen_cases as sc

K = prc.K
NUM_BASE = prc.NUM_BASE
MAX_PAIRS = 32
DEPTHS = (1, 2, 3, 5, 9, 17, 24, 31)
STOP = 1e30
FLAVOURS = ("double", "float")
CHANNELS = (0, 2)
SCALED = {"deep_up": 2.0 ** 40, "deep_down": 2.0 ** -40}
GROUPS = ("ramp", "deep", "mixed", "one", "with_row0") + tuple(SCALED)
ROW0_ROWS, ROW0_DECAY, ROW0_COHERENCE = 14, 0.4, 0.2      # `with_row0`: base rows per vector (row 0 among them), weights, see there
GROW = float(np.float32(1.000001))             # the kernel's float constants, as the values they are
RNORM_UP = float(np.float32(1.0000002))


def dtype_of(flavour):
    return np.float64 if flavour == "double" else np.float32


def group_vectors(base, name):
    """float64 [16, 64], f32-valued"""
    if name in SCALED:
        return pc.as_f32(prc.group_vectors(base, "deep") * SCALED[name])
    if name != "with_row0":
        return prc.group_vectors(base, name)
    # Base rows that are nearly orthogonal to each other (|<a, b>| < ROW0_COHERENCE) under weights that fall steeply: the pursuit
    # then takes more of them as base rows, one pair each (9 or 10 in some slots; the groups of pair_round_cases.py reach 8), before
    # the rows of the unlocked blocks, which lie close to many base rows, take over.
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    for i in range(16):
        rows = []
        for r in rng.permutation(np.arange(1, base.shape[0] - 1)):
            if all(abs(base[r] @ base[s]) < ROW0_COHERENCE for s in rows):
                rows.append(int(r))
            if len(rows) == ROW0_ROWS - 1:
                break
        rows.insert(1 + i % 3, 0)                           # row 0 is the second to fourth heaviest: a pair exists before it
        v = np.zeros(64)
        for j, r in enumerate(rows):
            v = v + 900.0 * ROW0_DECAY ** j * base[r]
        out.append(v)
    return pc.as_f32(np.array(out))


def group_quant(v, depth):
    """the group's tiny step everywhere, 1e30 at index `depth` (1 ... K - 1): the pursuit ends at step `depth` at the latest"""
    assert 0 < depth < K
    q = pc.tiny_quant(v, K)
    q[depth] = STOP
    return q


def zigzag(q):
    return ((q << 1) ^ (q >> 31)) & 0xFFFFFFFF


def round_away(x):
    """C's round(): to the nearest integer, halves away from zero.  x: a Python float (the difference below is exact)."""
    a = abs(x)
    f = float(np.floor(a))
    n = int(f) + (1 if a - f >= 0.5 else 0)
    return -n if x < 0 else n


def chain_dot(rows, r):
    """rows[n, 64] . r[64], both of the flavour's dtype -> [n]: tot = 0; tot += row[j] * r[j], j ascending, every product and sum
    rounded to the dtype (numpy multiplies elementwise and accumulates one after the other)"""
    assert rows.dtype == r.dtype and rows.dtype in (np.float32, np.float64)
    return np.cumsum(rows * r[None, :], axis=1, dtype=rows.dtype)[:, -1]


class Dictionary:
    """one channel's rows in the flavour's type"""

    def __init__(self, base, det_rows, det_ch, flavour):
        dt = dtype_of(flavour)
        self.flavour = flavour
        self.base = np.ascontiguousarray(base, np.float64).astype(dt)
        self.det = np.ascontiguousarray(det_ch, np.float64).astype(dt)
        self.rows = np.asarray(det_rows, np.int64)
        self.off = sc.row_offsets(self.rows)

    def block(self, blk):
        return self.det[self.off[blk]:self.off[blk] + self.rows[blk]]


class Pair:
    def __init__(self, created, block, rows, first):
        self.created, self.block, self.rows, self.first = created, block, rows, first     # first: its dictionary index

    def meta(self):
        return self.block | (self.rows << 9) | (self.first << 16)


class Replay:
    """One vector's pursuit.  ids: the chosen dictionary indices of the steps that went on (q != 0); r[s]: the residual entering
    step s (s = 0 ... count); q, c (Python floats, exact), sel (Gram row: base row, or 510 + detail row) and atom_block (block of a
    detail atom, -1 for a base row) per step; pairs in creation order; repeats: steps that chose a base row again."""

    def __init__(self, dic, v, quant, ids):
        dt = dtype_of(dic.flavour)
        self.count = len(ids)
        assert self.count < K                                  # never the K cap
        self.ids = list(ids)
        self.r = [np.ascontiguousarray(v, np.float64).astype(dt)]
        self.q, self.c, self.sel, self.atom_block, self.pairs, self.repeats = [], [], [], [], [], []
        self.unlock0 = None
        segments = []                                          # (first index, block) of every appended block, repeats included
        next_off, seen = NUM_BASE, set()
        for s, i in enumerate(self.ids):
            row, sel, blk = self._resolve(dic, segments, i)
            q, c = self.quantise(dic.flavour, chain_dot(row[None, :], self.r[s])[0], quant[s])
            assert q != 0, (s, i)
            self.q.append(q); self.c.append(float(c)); self.sel.append(sel); self.atom_block.append(blk)
            scaled = c * row                                   # Vector::Scale, then Vector::Subtract: two roundings
            self.r.append(self.r[s] - scaled)
            if i < NUM_BASE:
                rows = int(dic.rows[i])
                if i in seen:
                    self.repeats.append(s)
                elif i == 0:
                    self.unlock0 = s
                else:
                    self.pairs.append(Pair(s, i, rows, next_off))
                seen.add(i)
                segments.append((next_off, i))
                next_off += rows
        self.segments = segments

    @staticmethod
    def _resolve(dic, segments, i):
        if i < NUM_BASE:
            return dic.base[i], i, -1
        for first, blk in segments:
            if first <= i < first + dic.rows[blk]:
                drow = int(dic.off[blk]) + i - first
                return dic.det[drow], NUM_BASE + drow, blk
        raise IndexError(i)

    @staticmethod
    def quantise(flavour, p, step):
        dt = dtype_of(flavour)
        step = dt(step)
        q = round_away(float(dt(p) / step))
        return q, step * dt(q)

    def ending_q(self, dic, quant, end_id, e):
        """q of step e when it ends the pursuit (by `quant`), from the index its record names"""
        row, _, _ = self._resolve(dic, self.segments, end_id)
        return self.quantise(dic.flavour, chain_dot(row[None, :], self.r[e])[0], quant[e])[0]

    # ---- what a stop at `depth` leaves behind ----------------------------------------------------------
    def end(self, depth):
        return min(depth, self.count)

    def pairs_at(self, depth):
        return [p for p in self.pairs if p.created < self.end(depth)]

    def updates(self, pair, depth):
        """the steps whose choice updates `pair` before the pursuit ends at `depth`"""
        return range(pair.created + 1, self.end(depth))

    def items(self, step, depth):
        """pairs of the vector that the pair rounds at the end of `step` update"""
        return sum(1 for p in self.pairs if p.created < step) if step < self.end(depth) else 0


def replay_group(dic, v, ora, channel):
    """the group at the deepest stop: [(replay, oracle result)] per vector"""
    q = group_quant(v, DEPTHS[-1])
    out = []
    for i in range(v.shape[0]):
        res = ora.calc_mp(channel, v[i], quant=q)
        out.append((Replay(dic, v[i], q, prc.chosen_ids(res[0], res[1])), res))
    return out


# ---- the bound E, in float64 ----------------------------------------------------------------------------
def rnorm_model(r):
    """|r~| of the kernel's phase (2a): the 2-norm of the residual rounded to float, times 1.0000002f"""
    x = np.asarray(r, np.float64).astype(np.float32).astype(np.float64)
    return float(np.sqrt((x * x).sum())) * RNORM_UP


def bound_start(r):
    """E of a new pair: the MFMA bound of the residual it starts from"""
    return float(sc.reference_bound(np.asarray(r, np.float64)[None, :])[0])


def bound_grow(E, c, r):
    """E after the update by coefficient c of a step entered with residual r"""
    return (E + 2.0 ** -21 * (abs(float(np.float32(c))) + rnorm_model(r))) * GROW


def bound_model(rp, pair, depth):
    """(E in float64, number of updates) of `pair` when the pursuit has ended at `depth`"""
    E = bound_start(rp.r[pair.created + 1])
    steps = rp.updates(pair, depth)
    for j in steps:
        E = bound_grow(E, rp.c[j], rp.r[j])
    return E, len(steps)


# ---- the float fused multiply-add, exactly ------------------------------------------------------------------
def _nearest_f32(x):
    """Fraction -> the nearest float32, ties to the even significand"""
    g = np.float32(float(x))
    cands = {float(g), float(np.nextafter(g, np.float32(-np.inf))), float(np.nextafter(g, np.float32(np.inf)))}
    best = min(cands, key=lambda t: (abs(Fraction(t) - x), int(np.float32(t).view(np.uint32)) & 1))
    return np.float32(best)


def fma32(a, b, c):
    """fmaf(a, b, c) for a float32 scalar a and float32 arrays b, c: one rounding of the exact a * b + c.
    The product of two float32 is exact in float64; the sum in float64 is rounded once more than the fma rounds, which changes
    the float32 result only where that sum is exactly halfway between two float32 (any other double lies on the same side of every
    halfway point as the exact sum it was rounded from, the halfway points being doubles themselves): those are settled in
    rational arithmetic.  Finite values whose product neither overflows nor underflows float64."""
    a, b, c = np.float32(a), np.ascontiguousarray(b, np.float32), np.ascontiguousarray(c, np.float32)
    s = np.float64(a) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(np.float32)
    o64 = out.astype(np.float64)
    with np.errstate(over="ignore"):
        other = np.where(s > o64, np.nextafter(out, np.float32(np.inf)), np.nextafter(out, np.float32(-np.inf))).astype(np.float64)
    halfway = (s != o64) & (np.abs(s - o64) == np.abs(other - s))
    for k in np.argwhere(halfway):
        k = tuple(k)
        out[k] = _nearest_f32(Fraction(float(a)) * Fraction(float(b[k])) + Fraction(float(c[k])))
    return out
