"""Hand-made records for the tile decoder, shared by the host test and the device test (nothing here needs a GPU): record lists that
the container format and the reference's FromCoeffsDynamic allow and that no matching pursuit emits.

A frame is a list of records per tile-channel, written as (choice, q) with the choice absolute; `pack` turns them into the counts and
choice words the kernels read, ia.assemble_streams into a container.  Every tile-channel takes one of the CLASSES, cycling with
(tile + channel); a Half tile keeps its chroma empty, an Extreme list takes one of its turns in four and a Cancel list the others,
and a few tiles are set aside (`set_aside`) for lists in which U alone, or V alone, carries what a mistake in the dictionary would
change.  The seed is fixed; what the frames have to show with it, test_record_cases.py asserts.

The header tables are the frame's own: steps 0 and 1 are 8 and 1 in luma (a Half list needs them), steps 3 and 4 are 60000 and 59999
(a Cancel list needs them), steps 5 and 6 are 65535 and 0; every other step is small.  At K = 5 luma has no room for 65535 and 0, so
U and V carry them there instead of the Cancel pair.  A list that runs through a step of 59999 or more holds a zero coefficient
there (its choice still counts for the dictionary), and any coefficient at a step of 0.

`decode` restates the reference's tile decode (MatchingPursuit.cpp:109-128, misc.cpp:28-36) in numpy, with a `mutant=` switch for the
mistakes a decoder can make.  It exists only to show that the frames tell right from wrong: no expected pixel of any test comes
from it.  Two of the mutants need a word:
  clamp_before_round  swapping std::clamp and std::round alone is no mutant: both are monotone and the bounds are whole numbers, so
                      the result is the same for every input.  The switch clamps the luma sum to 0 ... 255 before RGBFromYUV instead,
                      the nearest mistake that can show.
  q_int16_wrap        the coefficient's zig-zag decode as -((zz + 1) >> 1) in 16-bit arithmetic: zz + 1 wraps for the symbol 0xFFFF,
                      which gives 0 instead of -32768."""
import functools

import numpy as np

NB = 510                                        # base atoms; the dynamic dictionary's first detail row
SEED = 20261032
FRAMES = {                                      # name: (width, height, K, closed)
    "small": (37, 21, 8, False),                # ragged both ways, 5 x 3 tiles
    "odd_k": (40, 24, 5, False),                # (K & 3) != 0
    "wide": (261, 277, 32, False),              # 33 x 35 = 1155 tiles: tile 1024 inside
    "wide_closed": (261, 277, 32, True),        # no forward reference: every prefix of every list decodes
}
CLASSES = ("flat", "half", "forward", "zero_unlock", "repeat", "edge", "extreme", "cancel", "empty")
MUTANTS = ("earlier_only", "no_repeat", "luma_detail", "quant_by_channel", "step0_zigzag", "half_even", "truncate", "no_clamp",
           "clamp_before_round", "q_int16_wrap")
BAD_KINDS = ("beyond", "negative", "first_detail")
# Tiles set aside, the same in every frame: one chroma channel alone carries detail rows and repeats (a list that is Forward and
# Repeat at once) over a flat luma of 128, which no mistake in the dictionary can touch and which keeps both signs of the chroma in
# range; and, where a frame can afford the black pixels, one tile with no record at all (the ragged corner tile of `small`).
SOLO = ((11, 1), (13, 2))                       # (tile, channel)
EMPTY_TILE = 14                                 # count 0 on all three channels; not in odd_k, where it would be 1/15 of the frame
# In a frame of more than 1100 tiles: the two classes that the Half tiles (chroma empty) always displace from a channel, and all of
# the tiles set aside once more BEHIND tile 1024, there with nothing but the one chroma channel live
DISPLACED = ((2, 1, "forward"), (5, 2, "zero_unlock"))
BEHIND = 1090
HALF_A = (17, 128, -2, 254, 60, 100, 0, 127, 160, 252, 200, 9, 230)
HALF_N = (0, -1, 1, 2)


def zigzag(v):
    v = int(v)
    return (v << 1) ^ (v >> 63)


def unzigzag(z):
    z = int(z)
    return (z >> 1) ^ -(z & 1)


def tables(K):
    """the header's steps [3, K] (u16)"""
    small = lambda ch, i: ((5, 4, 6)[ch] + (i * (7, 5, 3)[ch]) % (11, 13, 7)[ch])          # noqa: E731
    rows = [([8, (1, 3, 2)[ch], (16, 14, 18)[ch], 60000, 59999, 65535, 0] + [small(ch, i) for i in range(7, 32)])[:K] for ch in range(3)]
    if K < 7:
        rows[1][3:5] = [65535, 0]
        rows[2][3:5] = [0, 65535]
    return np.array(rows, np.uint16)


@functools.lru_cache(maxsize=None)
def dictionary():
    """(base[510, 64], det[3][rows, 64], det_rows[510], det_off[511]) of the oracle's context; none of it depends on K"""
    from oracle import oracle_py as oracle
    c = oracle.OracleContext(8, 8, 3.5)
    assert c.nbase == NB and set(np.unique(c.det_rows)) <= {62, 63}
    return c.base, c.det, c.det_rows.astype(np.int64), c.det_off.astype(np.int64)


def dictionary_size(choices):
    """rows of the dynamic dictionary that a list of choices builds: the base atoms and one block per base choice, repeats included"""
    rows = dictionary()[2]
    return NB + sum(int(rows[c]) for c in choices if 0 <= c < NB)


def outside(record_list):
    """the steps of a list whose choice lies outside the list's dynamic dictionary"""
    size = dictionary_size([c for c, _ in record_list])
    return [i for i, (c, _) in enumerate(record_list) if not 0 <= c < size]


def closed(record_list):
    """every prefix of the list decodes"""
    return all(not outside(record_list[:n]) for n in range(1, len(record_list) + 1))


# ---- the lists ------------------------------------------------------------------------------------------------------------------

class _List:
    """a list under construction: `add` takes the coefficient wanted (about 8 x the pixel amplitude) and finds q for the step's quantiser"""

    def __init__(self, quant, ch):
        self.steps, self.items = [int(s) for s in quant[ch]], []

    def add(self, choice, c=0.0, q=None):
        s = self.steps[len(self.items)]
        if q is None:
            if s == 0:
                q = 32767 if c >= 0 else -32768              # times 0: never seen
            elif s >= 59999:
                q = 0                                        # a zero coefficient: the choice still counts
            else:
                q = int(round(c / s))
                if q == 0 and c != 0:
                    q = 1 if c > 0 else -1
        self.items.append((int(choice), int(q)))
        return self

    def room(self):
        return len(self.steps) - len(self.items)


def _bases(rng, n):
    """n distinct base atoms, none of them 0"""
    return [int(b) for b in rng.choice(np.arange(1, NB), n, replace=False)]


def _amp(rng, lo=30, hi=100):
    return float(rng.integers(lo, hi)) * (1 if rng.random() < 0.5 else -1)


def _flat_c(rng, ch, turn=0):
    """the coefficient of base atom 0 (the constant 0.125): 8 x the level; a luma level outside 0 ... 255 on two turns in eight"""
    if ch == 0:
        return 8.0 * float({1: 270, 5: -15}.get(turn % 8, rng.integers(40, 221)))
    return 8.0 * float(rng.integers(-25, 26))


def _make_list(cls, rng, quant, ch, K, is_closed, state):
    rows = dictionary()[2]
    L = _List(quant, ch)
    variant = state[cls] = state.get(cls, -1) + 1
    if cls == "empty":
        return []
    if cls == "flat":
        state["flat", ch] = state.get(("flat", ch), -1) + 1
        return L.add(0, _flat_c(rng, ch, state["flat", ch])).items
    if cls == "half":
        if ch != 0:
            return []
        a, n = HALF_A[variant % len(HALF_A)], HALF_N[(variant // len(HALF_A) + variant) % len(HALF_N)]
        return L.add(0, q=a).add(0, q=4 * (2 * n + 1)).items
    if cls == "forward":
        b2, b3, b4 = _bases(rng, 3)
        if is_closed:                                        # the same rows, named after their blocks
            if variant % 2 == 0:
                return L.add(0, _flat_c(rng, ch)).add(b2, _amp(rng)).add(NB + rows[0] + int(rng.integers(0, rows[b2])), _amp(rng)).items
            return L.add(b2, _amp(rng)).add(0, _flat_c(rng, ch)).add(NB + rows[b2] + int(rng.integers(0, rows[0])), _amp(rng)).items
        if variant % 2 == 0:                                 # step 0 names a row of the fourth block
            x = NB + rows[0] + rows[b2] + rows[b3] + int(rng.integers(0, rows[b4]))
            return L.add(x, _amp(rng)).add(0, _flat_c(rng, ch)).add(b2, _amp(rng)).add(b3, _amp(rng)).add(b4, _amp(rng)).items
        x = NB + rows[0] + rows[b2] + int(rng.integers(0, rows[b3]))     # step 1 names a row of the third block
        return L.add(0, _flat_c(rng, ch)).add(x, _amp(rng)).add(b2, _amp(rng)).add(b3, _amp(rng)).items
    if cls == "solo":                                        # the second copy's rows named before the second choice of b
        (b,) = _bases(rng, 1)
        x = NB + rows[b] + int(rng.integers(0, rows[b] - 1))
        if is_closed:
            return L.add(b, _amp(rng)).add(b, _amp(rng, 8, 40)).add(x, _amp(rng)).items
        return L.add(x, _amp(rng)).add(b, _amp(rng)).add(NB + 2 * rows[b] - 1, _amp(rng)).add(b, _amp(rng, 8, 40)).items
    if cls == "zero_unlock":
        (b,) = _bases(rng, 1)
        if variant % 2 == 0:
            return L.add(0, _flat_c(rng, ch)).add(b, q=0).add(NB + rows[0] + int(rng.integers(0, rows[b])), _amp(rng)).items
        return L.add(b, q=0).add(0, _flat_c(rng, ch)).add(NB + int(rng.integers(0, rows[b])), _amp(rng)).items
    if cls == "repeat":
        b = 0 if ch == 0 else _bases(rng, 1)[0]              # luma repeats the constant, which keeps the tile in range
        first = _flat_c(rng, ch) if b == 0 else _amp(rng)
        if variant % 3 == 2 and K >= 8:                      # six copies of one block behind the constant's
            (b,) = _bases(rng, 1)
            L.add(0, _flat_c(rng, ch)).add(b, _amp(rng)).add(b, _amp(rng)).add(b).add(b).add(b).add(b, 1.0)
            return L.add(NB + rows[0] + 2 * rows[b] - 1, _amp(rng)).items
        L.add(b, first).add(b, _amp(rng, 8, 40))
        return L.add(NB + 2 * rows[b] - 1 if variant % 3 == 0 else NB, _amp(rng)).items
    if cls == "edge":
        kind = variant % 4
        if kind == 0:
            return L.add(0, _flat_c(rng, ch)).add(NB - 1, _amp(rng)).items
        if kind == 1:                                        # the last row of the whole dictionary
            (b,) = _bases(rng, 1)
            return L.add(0, _flat_c(rng, ch)).add(b, _amp(rng)).add(NB + rows[0] + rows[b] - 1, _amp(rng)).items
        if kind == 2:
            return L.add(0, _flat_c(rng, ch)).add(NB, _amp(rng)).items
        bases = [0] + _bases(rng, K - 2)                     # K - 1 distinct base choices, then the last row of the last block
        L.add(0, _flat_c(rng, ch))
        for b in bases[1:]:
            L.add(b, _amp(rng, 8, 30))
        return L.add(dictionary_size(bases) - 1, _amp(rng)).items
    if cls == "extreme":
        (b,) = _bases(rng, 1)
        q = -32768 if variant % 2 == 0 else 32767
        if 65535 in L.steps and variant % 3 != 0:            # q = +-1 at a step of 65535, behind zero coefficients
            L.add(0, _flat_c(rng, ch))
            while L.steps[len(L.items)] != 65535:
                L.add(b, _amp(rng, 8, 30))
            L.add(b, q=1 if variant % 2 else -1)
            if L.room() and L.steps[len(L.items)] == 0:
                L.add(b, q=q)
            return L.items
        return L.add(0, _flat_c(rng, ch)).add(b, q=q).items
    if cls == "cancel":
        if 60000 not in L.steps:
            return L.add(0, _flat_c(rng, ch)).items
        b, b2 = _bases(rng, 2)
        L.add(0, 8.0 * (128 if ch == 0 else int(rng.integers(-20, 21))))
        while L.steps[len(L.items)] != 60000:
            L.add(b2 if len(L.items) > 1 else 0, _amp(rng, 8, 40))
        return L.add(b, q=20).add(b, q=-20).items
    raise ValueError(cls)


def make_records(name):
    """records[t][ch] = [(choice, q), ...] of a frame"""
    W, H, K, is_closed = FRAMES[name]
    quant = tables(K)
    rng = np.random.default_rng(SEED + sorted(FRAMES).index(name.replace("_closed", "")))
    tiles = -(-W // 8) * -(-H // 8)
    state, records = {}, []
    for t in range(tiles):
        per_channel = []
        for ch in range(3):
            cls = CLASSES[(t + ch) % len(CLASSES)]
            if cls == "extreme":                             # one turn in four, for the cap on clamped samples: the others cancel
                state["turn"] = state.get("turn", 0) + 1
                if state["turn"] % 4 != 1:
                    cls = "cancel"
            if ch > 0 and CLASSES[t % len(CLASSES)] == "half":
                cls = "empty"                                # a Half tile: Y = a + n + 0.5 reaches the rounding as it is
            per_channel.append(_make_list(cls, rng, quant, ch, K, is_closed, state))
        records.append(per_channel)
    for t, ch, cls in set_aside(name):
        records[t] = [[], [], []]
        if cls:
            records[t][ch] = _make_list(cls, rng, quant, ch, K, is_closed, {})
        if cls == "solo" and t < BEHIND:
            records[t][0] = [(0, 128)]
    return records


def plain(lst):
    """a list that no mistake in the dynamic dictionary can touch: empty, or base atom 0 alone"""
    return not lst or (len(lst) == 1 and lst[0][0] == 0)


def set_aside(name):
    """(tile, channel, class) of the tiles that do not follow the cycle; class None: no record at all"""
    W, H, _, _ = FRAMES[name]
    tiles = -(-W // 8) * -(-H // 8)
    out = [(t, ch, "solo") for t, ch in SOLO] + ([] if name == "odd_k" else [(EMPTY_TILE, 0, None)])
    if tiles > 1100:
        out += list(DISPLACED)
        out += [(t + BEHIND, ch, cls) for t, ch, cls in out]
    return out


def pack(records, K):
    """records[t][ch] = [(choice, q), ...] -> counts[tiles, 3] (u16), choices[tiles, 3, K] (u32): low half the step-0 choice as it is,
    then zigzag(choice - prev); high half zigzag(q) & 0xFFFF"""
    tiles = len(records)
    counts = np.zeros((tiles, 3), np.uint16)
    choices = np.zeros((tiles, 3, K), np.uint32)
    for t, per_channel in enumerate(records):
        for ch, lst in enumerate(per_channel):
            assert len(lst) <= K
            counts[t, ch] = len(lst)
            prev = 0
            for i, (choice, q) in enumerate(lst):
                assert -32768 <= q <= 32767
                low = choice if i == 0 else zigzag(choice - prev)
                assert 0 <= low <= 0xFFFF, (t, ch, i, choice, prev)
                choices[t, ch, i] = low | ((zigzag(q) & 0xFFFF) << 16)
                prev = choice
    return counts, choices


class Frame:
    def __init__(self, name, W, H, K, records, bad_at=None):
        self.name, self.W, self.H, self.K, self.records, self.bad_at = name, W, H, K, records, bad_at
        self.quant = tables(K)
        self.tiles_x, self.tiles_y = -(-W // 8), -(-H // 8)
        self.counts, self.choices = pack(records, K)

    @functools.cached_property
    def container(self):
        import imageexperiments_amd as ia
        return bytes(ia.assemble_streams(self.W, self.H, self.K, 8, self.quant.astype(np.float64), self.counts, self.choices))

    def streams(self):
        """(lengths, codes[6K]) as the reference holds them: per channel and step the live tiles' choice deltas and coefficient
        symbols, the step-0 coefficients not differenced"""
        codes = [[] for _ in range(6 * self.K)]
        for t in range(len(self.records)):
            for ch in range(3):
                for i in range(int(self.counts[t, ch])):
                    word = int(self.choices[t, ch, i])
                    codes[2 * self.K * ch + 2 * i].append(word & 0xFFFF)
                    codes[2 * self.K * ch + 2 * i + 1].append(word >> 16)
        return self.counts.reshape(-1).copy(), [np.array(c, np.uint16) for c in codes]

    def tile_of(self, t):
        """(x, y, w, h) of tile t inside the frame"""
        tx, ty = divmod(t, self.tiles_y)
        return 8 * tx, 8 * ty, min(8, self.W - 8 * tx), min(8, self.H - 8 * ty)

    def tile_mask(self, tiles):
        """[H, W] bool: the pixels of these tiles"""
        m = np.zeros((self.H, self.W), bool)
        for t in tiles:
            x, y, w, h = self.tile_of(t)
            m[y:y + h, x:x + w] = True
        return m


@functools.lru_cache(maxsize=None)
def frame(name):
    W, H, K, _ = FRAMES[name]
    return Frame(name, W, H, K, make_records(name))


def dc_symbols_round_trip(f):
    """the step-0 coefficient symbols of consecutive live tiles of a channel lie within +-32767 of each other"""
    for ch in range(3):
        live = [zigzag(f.records[t][ch][0][1]) & 0xFFFF for t in range(len(f.records)) if f.records[t][ch]]
        if any(abs(a - b) > 32767 for a, b in zip([0] + live[:-1], live)):
            return False
    return True


# ---- frames with one record outside its dictionary ------------------------------------------------------------------------------

def bad_cases():
    """(kind, channel, last): each kind in each channel, and at the last step of a K-long list.  first_detail has no such variant:
    a list without a base choice has no record inside its dictionary but base choices."""
    return [(kind, ch, False) for kind in BAD_KINDS for ch in range(3)] + [(kind, None, True) for kind in ("beyond", "negative")]


@functools.lru_cache(maxsize=None)
def bad(name, kind, ch=0, last=False, lower=0):
    """a copy of frame `name` with one record replaced; .bad_at = (tile, channel, step).  lower: taken off the `beyond` index"""
    f = frame(name)
    records = [[list(lst) for lst in per_channel] for per_channel in f.records]
    solo = {t for t, _, _ in set_aside(name)}
    for t, per_channel in enumerate(records):
        if t in solo:
            continue
        for c, lst in enumerate(per_channel):
            if outside(lst) or (not last and c != ch):
                continue
            if kind == "first_detail":
                if len(lst) != 1:
                    continue
                step, choice = 0, NB
            else:
                # the last record of a list, a detail row: no other record's place depends on it
                if len(lst) < 2 or lst[-1][0] < NB or (len(lst) == f.K) != last:
                    continue
                step = len(lst) - 1
                choice = dictionary_size([x for x, _ in lst[:-1]]) - lower if kind == "beyond" else -1
            lst[step] = (choice, lst[step][1] or 5)
            return Frame(f"{name}-{kind}-{c}{'-last' if last else ''}{'-lowered' if lower else ''}", f.W, f.H, f.K, records, (t, c, step))
    raise LookupError((name, kind, ch, last))


# ---- the reference's tile decode, restated ----------------------------------------------------------------------------------------

def _round_half_away(x):
    whole = np.trunc(x)
    return np.where(np.abs(x - whole) >= 0.5, whole + np.sign(x), whole)


def _decode_list(lst, quant, ch, mutant):
    base, det, rows, off = dictionary()
    det_ch = det[0] if mutant == "luma_detail" else det[ch]
    choices = [c for c, _ in lst]

    def table(upto):
        out, seen = [base[a] for a in range(NB)], set()
        for c in choices[:upto]:
            if 0 <= c < NB and not (mutant == "no_repeat" and c in seen):
                seen.add(c)
                out.extend(det_ch[off[c]:off[c] + rows[c]])
        return out
    full = None if mutant == "earlier_only" else table(len(lst))
    acc = np.zeros(64)
    for i, (choice, q) in enumerate(lst):
        if mutant == "step0_zigzag":
            choice = choice - choices[0] + unzigzag(choices[0])
        if mutant == "q_int16_wrap" and q == -32768:
            q = 0
        step = float(quant.reshape(-1)[ch] if mutant == "quant_by_channel" else quant[ch, i])
        coeff = step * float(q)
        dyn = table(i) if full is None else full
        if not 0 <= choice < len(dyn):
            continue
        acc = acc + dyn[choice] * coeff                      # one rounding for the product, one for the sum
    return acc


def decode(f, mutant=None):
    """uint8 [H, W, 3]: FromCoeffsDynamic per tile-channel, RGBFromYUV per pixel"""
    assert mutant is None or mutant in MUTANTS
    out = np.zeros((f.tiles_y * 8, f.tiles_x * 8, 3), np.uint8)
    for t, per_channel in enumerate(f.records):
        Y, U, V = (_decode_list(lst, f.quant, ch, mutant).reshape(8, 8) for ch, lst in enumerate(per_channel))     # [dy, dx]
        if mutant == "clamp_before_round":
            Y = np.clip(Y, 0.0, 255.0)
        rgb = np.stack([Y + 1.13983 * V, Y - 0.39466 * U - 0.58060 * V, Y + 2.03211 * U], axis=-1)
        if mutant == "truncate":
            rgb = np.trunc(rgb)
        elif mutant == "half_even":
            rgb = np.rint(rgb)
        else:
            rgb = _round_half_away(rgb)
        if mutant == "no_clamp":
            rgb = rgb.astype(np.int64) & 0xFF                # a cast that wraps
        else:
            rgb = np.clip(rgb, 0.0, 255.0)
        tx, ty = divmod(t, f.tiles_y)
        out[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = rgb.astype(np.uint8)
    return out[:f.H, :f.W]
