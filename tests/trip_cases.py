"""Two hand-made frames whose streams take the device's block loops beyond one trip of 64 blocks, shared by the host tests and the
device tests (nothing here needs a GPU), with their expected values from numpy alone and a numpy model of the loops.

The loops (mp_unpack.hip, mp_entropy.hip) and what makes them trip twice:
  unpack carry         64 blocks of 2048 coded symbols: a packed stream of more than 131 072 coded symbols
  window unpack carry  the same from block k0 = s0 / 2048: such a stream entered in the middle
  DC carry             256 threads striding over the sums of blocks of 2048 expanded symbols: more than 524 288 symbols
  run-length plan      64 blocks of 4096 symbols: more than 262 144 symbols, a run across position 262 144

A: 4096 x 2112, K = 2 (135 168 tiles, 12 streams).  B: 8192 x 4160, K = 1 (532 480 tiles, 6 streams).  All tiles are live but a
random 1 % with one step fewer in one channel.  Stream i = 2 (channel K + step) + (0 choices, 1 coefficients); the coefficient
streams of step 0 (i % 2K == 1) are difference coded in the container and summed by the parser.

The expectation: the held streams themselves, sliced by ranks counted from the lengths; of a step-0 coefficient stream the wrapping
sums of what its 16-bit differences hold (stream_cases._dc_difference, then region_cases.dc_sum), never the held values."""
import functools

import numpy as np

import region_cases
import stream_cases

CHUNK = 0x8001                                  # a run is cut into chunks of this many symbols
UNPACK_BLOCK, ENT_BLOCK, TRIP, DC_THREADS = 2048, 4096, 64, 256
INTERVALS = (32, 100, 128)
PLAN_TRIP = TRIP * ENT_BLOCK                    # 262 144: where the run-length plan starts its next trip
EVERY = 3200                                    # coded positions that are checkpoints at every interval above
ALPHABET = 300

FRAMES = {"A": (4096, 2112, 2), "B": (8192, 4160, 1)}
# name -> (frame, rectangle, what it is for)
RECTS = {
    "A_far": ("A", (4000, 0, 96, 2112), "far"),             # enters the barely packed streams at k0 = 64
    "A_span": ("A", (2000, 0, 2096, 2112), "span"),         # k0 = 32 ... k1 = 66
    "B_span": ("B", (1000, 0, 7000, 4160), "span"),         # k0 = 31, four trips from an unaligned start
    "B_mid": ("B", (5120, 0, 1024, 4160), "far"),           # enters at the cut between two chunks of one run
    "B_far": ("B", (8000, 0, 192, 4160), "far"),
    "B_last": ("B", (8104, 0, 88, 4160), "far"),            # step-0 coefficients behind expanded block 256
    "B_dc": ("B", (8, 0, 8184, 4160), "dc"),                # out0 > 0, more than 256 expanded blocks to sum over
}


def rects_of(frame):
    return [(name, rect) for name, (f, rect, _) in RECTS.items() if f == frame]


# ---- run lengths in numpy ------------------------------------------------------------------------------------------------
def rle_encode(held):
    """runLengthEncode: maximal runs cut into chunks of at most 0x8001; a chunk of one symbol is the symbol, a longer one the
    symbol twice and the count of further copies"""
    held = np.asarray(held, np.uint16)
    if not len(held):
        return held
    edge = np.flatnonzero(np.concatenate([[True], held[1:] != held[:-1]]))
    length = np.diff(np.concatenate([edge, [len(held)]]))
    n_full, rest = length // CHUNK, length % CHUNK
    n_chunks = n_full + (rest > 0)
    value = np.repeat(held[edge], n_chunks)
    nth = np.arange(n_chunks.sum()) - np.repeat(np.cumsum(n_chunks) - n_chunks, n_chunks)
    size = np.where(nth < np.repeat(n_full, n_chunks), CHUNK, np.repeat(rest, n_chunks))
    emits = np.where(size == 1, 1, 3)
    at = np.cumsum(emits) - emits
    out = np.zeros(emits.sum(), np.uint16)
    out[at] = value
    more = size > 1
    out[at[more] + 1] = value[more]
    out[at[more] + 2] = size[more] - 2
    return out


def coded_form(as_coded, force=False):
    """(coded, packed) by the size rule `packed + 4 < size`; force: wherever the stream is not empty (legal for a decoder)"""
    coded, packed = [], []
    for s in as_coded:
        r = rle_encode(s)
        use = len(s) > 0 if force else len(r) + 4 < len(s)
        coded.append(r if use else np.asarray(s, np.uint16))
        packed.append(bool(use))
    return coded, packed


def roles(mem, s0, s1, state0, prev0):
    """runLengthDecode's machine over mem[s0:s1) entered in state0 (0 fresh, 1 value, 2 count) with prev0 in front of s0 ->
    (is_count[s1 - s0], the symbol in front of each, the state behind s1 - 1).  Only a symbol that equals the one in front of it
    can be a repeat, so the Python loop visits those alone."""
    v = np.asarray(mem[s0:s1]).astype(np.int64)
    n = len(v)
    before = np.concatenate([[int(prev0)], v[:-1]]) if n else v
    if n == 0:
        return np.zeros(0, bool), before, state0
    same = v == before
    if s0 == 0:
        same[0] = False                         # a stream's first symbol is always a value
    rep = [False] * (n + 2)                     # rep[i + 2]: symbol i repeats a value, so a count follows; [0], [1]: the entry
    rep[0], rep[1] = state0 == 0, state0 == 2   # fresh = behind a count, which is behind a repeat
    for i in np.flatnonzero(same).tolist():
        rep[i + 2] = not rep[i + 1] and not rep[i]
    state1 = 2 if rep[n + 1] else 0 if rep[n] else 1
    return np.array(rep[1:n + 1], bool), before, state1


def expand(mem, s0, s1, state0, prev0):
    """-> (expanded symbols, state behind)"""
    count, before, state1 = roles(mem, s0, s1, state0, prev0)
    v = np.asarray(mem[s0:s1]).astype(np.int64)
    return np.repeat(np.where(count, before, v), np.where(count, v, 1)).astype(np.uint16), state1


def aux_arrays(coded, packed, dc):
    """per coded position (one more at the end): out, prev, state, dc in front of it -- index2_cases.aux_of without its loop"""
    v = np.asarray(coded).astype(np.int64)
    n = len(v)
    if packed:
        count, before, _ = roles(v, 0, n, 0, 0)
    else:
        count, before = np.zeros(n, bool), np.concatenate([[0], v[:-1]])
    copies, value = np.where(count, v, 1), np.where(count, before, v)
    out = np.concatenate([[0], np.cumsum(copies)])
    state = np.zeros(n + 1, np.int64)
    if packed:
        state[:n] = np.where(count, 2, 1)
        state[0] = 0
        state[1:n][count[:-1]] = 0
        state[n] = 0 if n and count[-1] else 1
    prev = np.concatenate([[0], v]) if packed else np.zeros(n + 1, np.int64)
    sums = np.concatenate([[0], np.cumsum(copies * unzigzag(value))]) & 0xFFFF if dc else np.zeros(n + 1, np.int64)
    return out, prev, state, sums


def unzigzag(x):
    x = np.asarray(x).astype(np.int64)
    return (x >> 1) ^ -(x & 1)


# ---- the streams ------------------------------------------------------------------------------------------------------------
class _Build:
    """a stream from stretches without equal neighbours and from runs, with the coded position kept alongside"""

    def __init__(self, rng):
        self.rng, self.parts, self.exp, self.coded, self.last = rng, [], 0, 0, 0

    def filler(self, n):
        if n <= 0:
            assert n == 0, n
            return
        v = (self.last + np.cumsum(self.rng.integers(1, ALPHABET, n))) % ALPHABET      # every step is 1 ... 299: no equal neighbours
        self.parts.append(v)
        self.exp, self.coded, self.last = self.exp + n, self.coded + n, int(v[-1])

    def to_coded(self, pos):
        self.filler(pos - self.coded)

    def to_exp(self, pos):
        self.filler(pos - self.exp)

    def to_coded_mod(self, residue):
        self.filler((residue - self.coded) % EVERY)

    def run(self, n):
        self.last = (self.last + 1 + int(self.rng.integers(0, ALPHABET - 1))) % ALPHABET
        self.parts.append(np.full(n, self.last))
        self.exp += n
        self.coded += 3 * (n // CHUNK) + (0 if n % CHUNK == 0 else 1 if n % CHUNK == 1 else 3)

    def done(self, n):
        out = np.concatenate(self.parts).astype(np.uint16)
        assert len(out) == n == self.exp and len(rle_encode(out)) == self.coded
        return out


def _barely(n, rng, edges, long_run_at=None, tail=300):
    """no equal neighbours but for: a short run whose coded symbols straddle each coded position of `edges` (pos, symbols in front
    of it: 1 = the pair is cut, 2 = the count is the block's first symbol), a run of 0x8001 + 10 across expanded position
    `long_run_at`, and a last run long enough for the size rule"""
    b = _Build(rng)
    todo = sorted([(pos - front, "short") for pos, front in edges] + ([(long_run_at - 100, "long")] if long_run_at else []))
    for n_run, (pos, what) in enumerate(todo):
        if what == "long":
            b.to_exp(pos)
            b.run(CHUNK + 10)
        else:
            b.to_coded(pos)
            b.run(2 + n_run % 6)
    b.to_exp(n - tail)
    b.run(tail)
    return b.done(n)


def _cuts(n, rng, big):
    """runs of 0x8001 - 1, 0x8001, 0x8001 + 1 and (big) 2 x 0x8001, each followed by a run of 1 - 3, placed against a block edge of
    the coded stream and against checkpoints of every interval; none of them across a multiple of 262 144"""
    b = _Build(rng)
    b.to_coded(UNPACK_BLOCK - 2)
    b.run(CHUNK)                                # v v | count: the count is block 1's first symbol
    b.run(1)
    b.to_coded_mod(EVERY - 1)
    b.run(CHUNK + 1)                            # the second v is a checkpoint: entered in state 1, inside the run
    b.run(2)
    b.to_coded_mod(EVERY - 2)
    b.run(CHUNK - 1)                            # the count is a checkpoint: state 2
    b.run(3)
    if big:
        b.to_exp(289000)
        b.to_coded_mod(EVERY - 3)
        b.run(2 * CHUNK)                        # the second chunk's first v is a checkpoint: state 0, inside the run
        b.run(1)
        b.to_exp(454000)
        b.to_coded_mod(EVERY - 2)
        b.run(2 * CHUNK)                        # the first count is a checkpoint: state 2, two chunks to expand from there
        b.run(3)
    b.to_exp(n)
    return b.done(n)


def _collide(n, rng):
    """v repeated v + 2 times (coded v v v), and runs whose count is the next run's value (a a c c ...)"""
    values, lengths, total = [], [], 0
    while total < n:
        kind = int(rng.integers(0, 3))
        v = int(rng.integers(0, 40))
        if kind == 0:
            add = [(v, v + 2)]
        elif kind == 1:
            c = int(rng.integers(0, 40))
            add = [(v, c + 2), (c, int(rng.integers(1, 4)))]
        else:
            add = [(v, int(rng.integers(1, 4)))]
        values += [a for a, _ in add]
        lengths += [m for _, m in add]
        total += sum(m for _, m in add)
    return np.repeat(values, lengths)[:n].astype(np.uint16)


def _short(n, rng):
    m = n // 2 + 8
    return np.repeat(rng.integers(0, 6, m), rng.integers(1, 9, m))[:n].astype(np.uint16)


def _boundaries_at(s, positions):
    """the stream with a run boundary exactly at each of `positions`"""
    for pos in positions:
        if pos < len(s) and s[pos - 1] == s[pos]:
            s[pos - 1] = (int(s[pos]) + 1) % 50
    return s


def _walk(n, rng):
    """a walk with flat stretches from near 65 500 (the 16-bit values wrap), a few steps beyond +-32 767 (their differences lose
    a bit in the container), and steps 1 then 2 in front of and at every multiple of 262 144: a run boundary exactly at the plan's trips"""
    steps = np.where(rng.random(n) < 0.12, rng.integers(-3, 4, n), 0).astype(np.int64)
    far = rng.choice(n, min(24, n), replace=False)
    steps[far] = rng.choice([-50000, -40000, 33000, 40000, 60000], len(far))
    for edge in range(PLAN_TRIP, n, PLAN_TRIP):
        steps[edge - 1], steps[edge] = 1, 2
    return ((65500 + np.cumsum(steps)) & 0xFFFF).astype(np.uint16)


def _kinds(name):
    if name == "A":
        edge = TRIP * UNPACK_BLOCK
        return {0: lambda n, r: _barely(n, r, [(edge, 1)]), 2: lambda n, r: _cuts(n, r, False), 3: _collide, 4: _short,
                8: lambda n, r: _barely(n, r, [(edge, 2)], tail=1000)}
    # B: the whole unpack trips at coded blocks 64, 128, 192; the window of B_span (k0 = 31) at 95, 159, 223
    edges = [(64 * 2048, 2), (95 * 2048, 1), (128 * 2048, 1), (159 * 2048, 2), (192 * 2048, 2), (223 * 2048, 1)]
    return {0: lambda n, r: _barely(n, r, edges, long_run_at=TRIP * ENT_BLOCK),
            2: lambda n, r: _cuts(n, r, True),
            4: lambda n, r: _boundaries_at(np.concatenate([_collide(n // 2, r), _short(n - n // 2, r)]), (PLAN_TRIP, 2 * PLAN_TRIP))}


@functools.lru_cache(maxsize=None)
def frame(name):
    """dict(W, H, K, counts, as_held, as_coded, want): want[i] = what every parse must give for stream i"""
    W, H, K = FRAMES[name]
    tiles = (W // 8) * (H // 8)
    rng = np.random.default_rng([20251021, ord(name)])
    counts = np.tile(np.array([K, 1, 1], np.uint16), (tiles, 1))
    fewer = rng.choice(tiles, tiles // 100, replace=False)
    counts[fewer, rng.integers(0, 3, len(fewer))] -= 1
    if name == "A":
        counts[:, 1] = np.minimum(counts[:, 1], 1)
        counts[77777, 1] = 2                                        # (channel 1, step 1) holds one symbol, (2, 1) none
    kinds = _kinds(name)
    held = []
    for i in range(6 * K):
        ch, step = (i // 2) // K, (i // 2) % K
        n = int((counts[:, ch] > step).sum())
        r = np.random.default_rng([20251021, ord(name), i])
        if i % (2 * K) == 1:
            held.append(_walk(n, r))
        elif n <= 1:
            held.append(np.full(n, 17 + i, np.uint16))
        else:
            held.append(kinds[i](n, r))
        assert len(held[-1]) == n
    coded = list(held)
    want = list(held)
    for i in (1, 2 * K + 1, 4 * K + 1):
        coded[i] = stream_cases._dc_difference(held[i]) if len(held[i]) else held[i]
        want[i] = region_cases.dc_sum(coded[i])
    return dict(W=W, H=H, K=K, bs=8, tiles=tiles, counts=counts.reshape(-1), as_held=held, as_coded=coded, want=want,
                quant=stream_cases.quant(K))


@functools.lru_cache(maxsize=None)
def container(name):
    import imageexperiments_amd as ia
    f = frame(name)
    return bytes(ia.write_compressed(f["W"], f["H"], f["K"], 8, f["quant"], f["counts"], f["as_held"]))


@functools.lru_cache(maxsize=None)
def index(name, interval):
    import imageexperiments_amd as ia
    return bytes(ia.container_index(container(name), interval, expanded=True))


@functools.lru_cache(maxsize=None)
def packed_form(name):
    """(coded, packed) of the frame's streams by the size rule, from numpy"""
    return coded_form(frame(name)["as_coded"])


def is_dc(i, K):
    return i % (2 * K) == 1


def ranges_of(name, rect):
    f = frame(name)
    K = f["K"]
    t0, t1, _ = region_cases.tile_range(rect, f["H"])
    c = f["counts"].reshape(-1, 3)
    ranges = np.zeros((3 * K, 2), np.uint64)
    for ch in range(3):
        for step in range(K):
            ranges[ch * K + step] = ((c[:t0, ch] > step).sum(), (c[:t1, ch] > step).sum())
    return ranges


def expected_window(name, rect):
    """(symbols, ranges[3K, 2]): the lengths whole, then [r0, r1) of every expected stream"""
    f = frame(name)
    ranges = ranges_of(name, rect)
    parts = [f["counts"]] + [f["want"][i][int(ranges[i // 2, 0]):int(ranges[i // 2, 1])] for i in range(6 * f["K"])]
    return np.concatenate(parts), ranges


def expected_whole(name):
    f = frame(name)
    return np.concatenate(f["want"])


def expected_serial(name):
    """parse_container_by_index's symbols: the lengths, then the streams as coded"""
    return np.concatenate([frame(name)["counts"]] + packed_form(name)[0])


def first_difference(got, want, sizes, lengths_first=False):
    """None, or the first differing stream and position of two concatenations of streams of these sizes (lengths_first: behind
    the lengths stream, as the windowed parse gives them)"""
    if got.shape != want.shape:
        return f"{got.shape} symbols, expected {want.shape}"
    if np.array_equal(got, want):
        return None
    at = int(np.flatnonzero(got != want)[0])
    off = np.cumsum([0] + list(sizes))
    stream = int(np.searchsorted(off, at, side="right")) - 1
    name = "the lengths" if lengths_first and stream == 0 else f"stream {stream - (1 if lengths_first else 0)}"
    return f"first difference at symbol {at}: {name} position {at - off[stream]}: {got[at]} != {want[at]}"


def window_sizes(name, ranges):
    """the sizes of what the windowed parse returns: the lengths, then [r0, r1) of each of the 6K streams"""
    return [len(frame(name)["counts"])] + [int(b) - int(a) for a, b in np.repeat(ranges, 2, axis=0)]


# ---- the window of every stream that is cut, from the host's index ------------------------------------------------------------
def windows(ia, name, rect, interval):
    """[dict(i, dc, packed, c0, c1, n_chunks, s0, s1, k0, k1, state0, state1, out0, out1, prev0, dc0)] of the streams with aux entries
    whose window is not empty, from the host's index and window_chunks_by_index"""
    f = frame(name)
    K = f["K"]
    blob, v2 = container(name), index(name, interval)
    chunks, route = ia.window_chunks_by_index(blob, v2, rect)
    assert route == 0
    info = ia.index_info(v2)["streams"]
    out = []
    for i in range(6 * K):
        s = info[i + 1]
        dc = is_dc(i, K)
        c0, c1 = int(chunks[i, 0]), int(chunks[i, 1])
        if not (s["packed"] or dc) or c0 >= c1:
            continue
        aux = ia.index_aux(v2, i + 1)
        n = len(aux["out"])
        s0, s1 = c0 * interval, min(c1 * interval, int(s["n_coded"]))
        w = dict(i=i, dc=dc, packed=bool(s["packed"]), c0=c0, c1=c1, n_chunks=n, s0=s0, s1=s1, k0=s0 // UNPACK_BLOCK,
                 k1=-(-s1 // UNPACK_BLOCK), state0=int(aux["state"][c0]), out0=int(aux["out"][c0]), prev0=int(aux["prev"][c0]),
                 dc0=int(aux["dc"][c0]), check=c1 < n, n_coded=int(s["n_coded"]), expect=int(s["expect"]))
        w["state1"], w["out1"], w["prev1"], w["dc1"] = ((int(aux["state"][c1]), int(aux["out"][c1]), int(aux["prev"][c1]), int(aux["dc"][c1]))
                                                        if c1 < n else (None, w["expect"], None, None))
        out.append(w)
    return out


def _in_long_run(held, pos):
    """pos lies strictly inside a held run of 0x8001 symbols or more"""
    if pos <= 0 or pos >= len(held) or held[pos - 1] != held[pos]:
        return False
    differs = np.flatnonzero(held != held[pos])
    lo = differs[differs < pos].max() + 1 if (differs < pos).any() else 0
    hi = differs[differs > pos].min() if (differs > pos).any() else len(held)
    return hi - lo >= CHUNK


def check_coverage(ia):
    """what the frames are there for, from the host's index and chunk table: a changed builder fails here instead of testing nothing"""
    seen_entry, seen_exit, inside_long, dc_spans, dc_far = set(), set(), set(), 0, 0
    for name in FRAMES:
        f = frame(name)
        K = f["K"]
        got = ia.read_compressed(container(name), coded=True)
        coded, packed = packed_form(name)
        assert [bool(p) for p in got["packed"]] == packed, name        # every packed flag the cases rely on
        assert all(np.array_equal(a, b) for a, b in zip(got["codes"], coded)), name
        assert all(packed[i] for i in range(6 * K) if len(f["as_held"][i]) > 1), name
        sizes = sorted(len(s) for s in f["as_held"])
        assert name != "A" or sizes[:4] == [0, 0, 1, 1]                # an empty pair and a pair of one symbol
        blocks = {i: -(-len(coded[i]) // UNPACK_BLOCK) for i in range(6 * K) if packed[i] and not is_dc(i, K)}
        assert max(blocks.values()) >= (66 if name == "A" else 130), blocks
        for rect_name, rect in rects_of(name):
            what = RECTS[rect_name][2]
            for interval in INTERVALS:
                ws = windows(ia, name, rect, interval)
                plain = [w for w in ws if w["packed"] and not w["dc"]]
                if what == "far":
                    assert any(w["k0"] >= TRIP for w in plain), (rect_name, interval)
                if what == "span":
                    assert any(0 < w["k0"] < TRIP < w["k1"] and w["k0"] % TRIP for w in plain), (rect_name, interval)
                    assert name != "B" or any(w["k1"] - w["k0"] > 2 * TRIP for w in plain), (rect_name, interval)
                for w in ws:
                    if w["c0"] > 0 and w["packed"]:
                        seen_entry.add(w["state0"])
                        if not w["dc"] and _in_long_run(f["as_held"][w["i"]], w["out0"]):
                            inside_long.add(w["state0"])
                    if w["c1"] < w["n_chunks"] and w["packed"]:
                        seen_exit.add(w["state1"])
                    if w["dc"] and w["out0"] > 0 and w["out1"] // UNPACK_BLOCK - w["out0"] // UNPACK_BLOCK > DC_THREADS:
                        dc_spans += 1
                    if w["dc"] and w["out0"] // UNPACK_BLOCK >= DC_THREADS:
                        dc_far += 1
    assert seen_entry == {0, 1, 2} and seen_exit == {0, 1, 2}, (seen_entry, seen_exit)
    assert inside_long == {0, 1, 2}, inside_long                    # entries strictly inside a run of 0x8001 or more, in every state
    assert dc_spans >= 3 and dc_far >= 3, (dc_spans, dc_far)
    # a run of 0x8001 or more across expanded position 262 144 (entropy blocks 63 | 64), across a 2048-block edge of the coded
    # stream and across a checkpoint of every interval
    b = frame("B")["as_held"]
    assert _in_long_run(b[0], TRIP * ENT_BLOCK)
    for name in FRAMES:
        cuts = packed_form(name)[0][2]
        assert cuts[UNPACK_BLOCK - 1] == cuts[UNPACK_BLOCK - 2] and cuts[UNPACK_BLOCK] == CHUNK - 2
        out = aux_arrays(cuts, True, False)[0]
        at = [p for p in range(EVERY, len(cuts), EVERY) if _in_long_run(frame(name)["as_held"][2], int(out[p]))]
        assert len(at) >= (3 if name == "B" else 1), (name, at)
    # every other stream of B has a run boundary exactly at the plan's trips: a plan that loses its carry there changes stream 0 alone
    for i, s in enumerate(frame("B")["as_coded"]):
        assert s[2 * PLAN_TRIP - 1] != s[2 * PLAN_TRIP] and (i == 0 or s[PLAN_TRIP - 1] != s[PLAN_TRIP]), i


# ---- the loops restated: blocks, trips, and what is carried between trips -----------------------------------------------------
WINDOW_VARIANTS = ("state_lost", "run_lost", "from_block_0", "entry_state_0", "prev0_zero", "prev0_memory", "out0_dropped",
                   "exit_unchecked")
DC_VARIANTS = ("dc0_dropped", "dc_carry_256")
PLAN_VARIANTS = ("chunk_cut_ignored", "run_before_lost", "out_before_lost")


def window_model(mem, w, variant=None, block=UNPACK_BLOCK, trip=TRIP):
    """mp_unpack_window_map / carry / fill over the coded symbols mem[0, n_coded) of which only [s0, s1) are the stream's (the
    rest is whatever the memory held): -> the stream's expanded positions [out0, out1) as an array, or None where the carry
    refuses (stream_ok = 0: nothing is written).  w: a dict as windows() gives; the whole stream is s0 = 0, state0 = 0, out0 = 0,
    s1 = n_coded, check False.  variant: one of WINDOW_VARIANTS, a loop that is subtly wrong."""
    s0, s1 = w["s0"], w["s1"]
    k0, k1 = s0 // block, -(-s1 // block)
    prev0 = 0 if variant == "prev0_zero" else int(mem[s0 - 1]) if variant == "prev0_memory" and s0 else w["prev0"]
    state = 0 if variant == "entry_state_0" else w["state0"]
    run = 0 if variant == "out0_dropped" else w["out0"]
    pieces = {}
    first = 0 if variant == "from_block_0" else k0
    for base in range(first, k1, trip):
        st, at = state, run
        for k in range(base, min(base + trip, k1)):
            # a block in front of k0 was never mapped: its piece is the one an earlier, whole unpack left there
            lo, hi = (max(s0, k * block), min(s1, (k + 1) * block)) if k >= k0 else (k * block, (k + 1) * block)
            symbols, behind = expand(mem, lo, hi, st, prev0 if lo == s0 else int(mem[lo - 1]))
            if k >= k0:
                pieces[k] = (at, symbols)
            st, at = behind, at + len(symbols)
        run = at - run if variant == "run_lost" and base > first else at   # lost: a later trip's own symbols alone
        if variant != "state_lost":
            state = st
    ok = run == w["out1"]
    if w["check"] and variant != "exit_unchecked":
        ok = ok and state == w["state1"] and int(mem[s1 - 1]) == w["prev1"]
    if not ok:
        return None
    out = np.full(w["out1"] - w["out0"], 0xFFFF, np.uint16)         # 0xFFFF: a position nobody wrote (no stream here holds it)
    for at, symbols in pieces.values():
        lo, hi = max(at, w["out0"]), min(at + len(symbols), w["out1"])
        if lo < hi:
            out[lo - w["out0"]:hi - w["out0"]] = symbols[lo - at:hi - at]
    return out


def whole(coded, expect):
    return dict(s0=0, s1=len(coded), state0=0, prev0=0, out0=0, out1=expect, check=False, dc0=0)


def dc_model(expanded, w, variant=None, block=UNPACK_BLOCK, threads=DC_THREADS):
    """mp_unpack_window_dc_sum / dc_scan over positions [out0, out1) of a step-0 coefficient stream's expanded differences (an
    array of the whole stream's size; positions outside are never read): the sums of the blocks in front of each block, from the
    one that holds out0, added up by `threads` threads striding, seeded with dc0"""
    out0, out1 = w["out0"], w["out1"]
    z = unzigzag(expanded[out0:out1])
    first, last = out0 // block, -(-out1 // block)
    part = np.zeros(last, np.int64)
    np.add.at(part, np.arange(out0, out1) // block, z)
    got = np.zeros(out1 - out0, np.int64)
    for d in range(first, last):
        upto = min(d, first + threads) if variant == "dc_carry_256" else d
        carry = int(part[first:upto].sum()) + (0 if variant == "dc0_dropped" else w["dc0"])
        lo, hi = max(out0, d * block), min(out1, (d + 1) * block)
        got[lo - out0:hi - out0] = carry + np.cumsum(z[lo - out0:hi - out0])
    return (got & 0xFFFF).astype(np.uint16)


def _emitted_span(p0, n, run_end, cut):
    """rle_emitted_span: symbols written for offsets [p0, p0 + n) of one run"""
    if n == 0:
        return 0
    hi = p0 + n
    if not cut:
        return (p0 <= 0 < hi) + (p0 <= 1 < hi) + (1 if run_end and hi - 1 >= 1 else 0)
    below = lambda x, r: (x + CHUNK - 1 - r) // CHUNK                # noqa: E731  offsets below x that are r mod CHUNK
    e = sum(below(hi, r) - below(p0, r) for r in (0, 1, CHUNK - 1))
    c = (hi - 1) % CHUNK
    return e + (1 if run_end and c >= 1 and c != CHUNK - 1 else 0)


def plan_model(raw, variant=None, block=ENT_BLOCK, trip=TRIP):
    """ent_runs_kernel<false> and ent_rle_plan_kernel: per block the symbols in front of its first run boundary (they belong to a
    run that began earlier), what the runs that begin inside it emit, and its last run's symbols; a wave walks the blocks 64 at a
    time and carries run_before and out_before -> the packed size the plan arrives at"""
    raw = np.asarray(raw).astype(np.int64)
    n = len(raw)
    cut = variant != "chunk_cut_ignored"
    starts = np.concatenate([[True], raw[1:] != raw[:-1]]) if n else np.zeros(0, bool)
    ends = np.concatenate([raw[1:] != raw[:-1], [True]]) if n else starts
    nb = -(-n // block)
    run_before = out_before = 0
    for base in range(0, nb, trip):
        val, total = run_before, 0
        for lb in range(base, min(base + trip, nb)):
            lo, hi = lb * block, min(n, (lb + 1) * block)
            size = hi - lo
            at = np.flatnonzero(starts[lo:hi])
            lead = int(at[0]) if len(at) else size
            lead_end = lead > 0 and bool(ends[lo + lead - 1])
            inner = 0
            if len(at):
                p = np.arange(lead, size) - np.repeat(at, np.diff(np.concatenate([at, [size]])))
                c = p % CHUNK if cut else p
                inner = int(((c <= 1).astype(np.int64) + ((c >= 1) & (ends[lo + lead:hi] | (cut & (c == CHUNK - 1))))).sum())
            carry = val if lead > 0 else 0
            total += inner + _emitted_span(carry, lead, lead_end, cut)
            val = size - int(at[-1]) if len(at) else val + size
        out_before = total if variant == "out_before_lost" else out_before + total
        run_before = 0 if variant == "run_before_lost" else val
    return out_before


# ---- named smallest cases: each wrong variant changes one of them, and none that is smaller ------------------------------------
def _stream(parts):
    """(held, coded) from (what, n): "f" a stretch without equal neighbours up to coded position n, "r" a run of n"""
    b = _Build(np.random.default_rng(5))
    for what, n in parts:
        b.to_coded(n) if what == "f" else b.run(n)
    held = b.done(b.exp)
    return held, rle_encode(held)


def _window_case(parts, s0=0, s1=None, stale=0xA5A5):
    """stale: what the memory outside [s0, s1) holds; None = the stream's own symbols, left by an earlier whole parse"""
    held, coded = _stream(parts)
    out, prev, state, _ = aux_arrays(coded, True, False)
    s1 = len(coded) if s1 is None else s1
    w = dict(s0=s0, s1=s1, state0=int(state[s0]), prev0=int(prev[s0]), out0=int(out[s0]), out1=int(out[s1]), check=s1 < len(coded),
             state1=int(state[s1]), prev1=int(prev[s1]), dc0=0)
    mem = coded.copy()
    if stale is not None:
        mem[:s0] = stale                                             # nobody parsed the symbols outside [s0, s1)
        mem[s1:] = stale
    return dict(mem=mem, w=w, want=held[w["out0"]:w["out1"]])


EDGE = TRIP * UNPACK_BLOCK


@functools.lru_cache(maxsize=None)
def window_cases():
    """name -> dict(mem, w, want), in order of size"""
    tail = [("f", EDGE + 1500), ("r", 40)]
    out = {
        "one_trip": _window_case([("f", EDGE - UNPACK_BLOCK - 1), ("r", 5), ("f", EDGE - 40), ("r", 40)]),   # 64 blocks, a pair across blocks 62 | 63
        "two_trips": _window_case(tail),                                                    # 65 blocks, nothing at the edge
        "pair_across_trips": _window_case([("f", EDGE - 1), ("r", 5)] + tail),              # v | v 3: block 64 is entered in state 1
        "count_across_trips": _window_case([("f", EDGE - 2), ("r", 9)] + tail),             # v v | 7: entered in state 2
    }
    inner = [("f", 40), ("r", 6), ("f", 100), ("r", 6), ("f", 300)]                       # v v 4 at 40, 41, 42
    out["enter_at_0"] = _window_case(inner, 0, 128)
    out["enter_fresh"] = _window_case(inner, 43, 128)
    out["enter_value"] = _window_case(inner, 41, 128)                                       # s0 is the second v: state 1, prev0 = v
    out["enter_count"] = _window_case(inner, 42, 128)
    held, coded = _stream(inner)
    out["enter_value_memory_equal"] = _window_case(inner, 60, 128, stale=int(coded[60]))    # the memory in front of s0 holds s0's symbol
    out["enter_block_64"] = _window_case([("f", EDGE + 1000), ("r", 4), ("f", EDGE + 4000)], EDGE + 96, EDGE + 3200, stale=None)
    return out


WINDOW_SMALLEST = {
    "state_lost": "pair_across_trips",
    "run_lost": "two_trips",
    "from_block_0": "enter_block_64",
    "entry_state_0": "enter_value",
    "prev0_zero": "enter_value",
    "prev0_memory": "enter_value",
    "out0_dropped": "enter_fresh",
    "exit_unchecked": "enter_at_0",
}
# cases of the same kind that come before the smallest one and must not show the variant
WINDOW_SMALLER = {
    "state_lost": ("one_trip", "two_trips"),
    "run_lost": ("one_trip",),
    "from_block_0": ("enter_at_0", "enter_fresh"),
    "entry_state_0": ("enter_at_0", "enter_fresh"),
    "prev0_zero": ("enter_at_0", "enter_fresh"),
    "prev0_memory": ("enter_at_0", "enter_fresh"),
    "out0_dropped": ("enter_at_0",),
    "exit_unchecked": (),
}


@functools.lru_cache(maxsize=None)
def dc_cases():
    """name -> dict(expanded differences, w, want)"""
    rng = np.random.default_rng(6)

    def case(n, out0, out1):
        z = rng.integers(0, 9, n).astype(np.uint16)
        sums = np.cumsum(unzigzag(z))
        w = dict(out0=out0, out1=out1, dc0=int(sums[out0 - 1]) & 0xFFFF if out0 else 0)
        return dict(expanded=z, w=w, want=(sums[out0:out1] & 0xFFFF).astype(np.uint16))
    blocks = DC_THREADS * UNPACK_BLOCK
    return {"from_0": case(5000, 0, 5000), "window": case(5000, 2100, 4500), "blocks_256": case(blocks + 2048, 0, blocks + 2048),
            "blocks_257": case(blocks + 2049, 0, blocks + 2049), "window_far": case(blocks + 9000, 2048 + 7, blocks + 8000)}


DC_SMALLEST = {"dc0_dropped": "window", "dc_carry_256": "blocks_257"}
DC_SMALLER = {"dc0_dropped": ("from_0",), "dc_carry_256": ("from_0", "window", "blocks_256")}


@functools.lru_cache(maxsize=None)
def plan_cases():
    """name -> the symbols the entropy stage is handed"""
    edge = TRIP * ENT_BLOCK
    return {
        "one_chunk": _stream([("f", 100), ("r", CHUNK), ("f", 200)])[0],
        "chunk_and_5": _stream([("f", 100), ("r", CHUNK + 5), ("f", 200)])[0],
        "blocks_64": _stream([("f", edge - 50), ("r", 50)])[0],
        "blocks_65": _stream([("f", edge), ("r", 9), ("f", edge + 100)])[0],              # a run boundary exactly at the trip
        "run_across_trips": _stream([("f", edge - 100), ("r", CHUNK + 10), ("f", edge + 50)])[0],
    }


PLAN_SMALLEST = {"chunk_cut_ignored": "chunk_and_5", "run_before_lost": "run_across_trips", "out_before_lost": "blocks_65"}
PLAN_SMALLER = {"chunk_cut_ignored": ("one_chunk",), "run_before_lost": ("one_chunk", "chunk_and_5", "blocks_64", "blocks_65"),
                "out_before_lost": ("one_chunk", "chunk_and_5", "blocks_64")}


FLIP_RECT, FLIP_INTERVAL = "B_span", 100


def far_exit_flips(ia):
    """[(what, damaged version-2 index of B)]: one flipped bit in out, prev, state and dc of entry c1 of B_span's window into a
    packed stream and into a step-0 coefficient stream, both left behind coded block 64"""
    import index2_cases
    name, rect, _ = RECTS[FLIP_RECT]
    blob, v2 = container(name), index(name, FLIP_INTERVAL)
    v1 = ia.container_index(blob, FLIP_INTERVAL)
    ws = [w for w in windows(ia, name, rect, FLIP_INTERVAL) if w["packed"] and w["check"] and w["k1"] > TRIP]
    picked = [w for w in ws if not w["dc"]][:1] + [w for w in ws if w["dc"]][:1]
    assert len(picked) == 2
    out = []
    for w in picked:
        at = 8 * index2_cases.aux_entry_offset(ia, v2, v1, w["i"] + 1, w["c1"])
        fields = [("out", at + 0), ("out", at + 3), ("prev", at + 64 + 0), ("prev", at + 64 + 9), ("state", at + 64 + 32), ("state", at + 64 + 33)]
        if w["dc"]:
            fields += [("dc", at + 64 + 16), ("dc", at + 64 + 27)]
        out += [(f"stream {w['i']} entry {w['c1']} {field} bit {bit - at}", index2_cases.flip(v2, bit)) for field, bit in fields]
    return out
