"""Frames, rectangles and expected values of index version 2's tests, shared by the host tests and the device tests (nothing
here needs a GPU): the aux entries and the chunk rule restated in numpy, from the serial coded parse alone."""
import functools

import numpy as np

import parse_cases
import region_cases
from region_cases import ACROSS_1024

F1_INTERVALS = region_cases.INTERVALS                               # 32, 100 and 0 = the default
DEFAULT_INTERVAL = 128
F2_SHAPE = (1003, 517, 103)                                         # oracle.synth_frame's arguments; K = 32, quality 3.5
F2_K, F2_QUALITY, F2_INTERVAL = 32, 3.5, 100
F2_INNER = (500, 250, 131, 77)
F2_RECTS = ((0, 0, 1003, 517), F2_INNER, (995, 3, 8, 514))


def f1():
    return region_cases.container()


@functools.lru_cache(maxsize=None)
def f2_frame():
    from oracle import oracle_py as oracle
    return oracle.synth_frame(*F2_SHAPE)


@functools.lru_cache(maxsize=None)
def f2():
    """the frame of test_eight_gather_blocks encoded by the oracle on the CPU"""
    from oracle import oracle_py as oracle
    return bytes(oracle.OracleContext(F2_K, 8, F2_QUALITY).encode_image(f2_frame()))


def zigzag(v):
    x = np.asarray(v).astype(np.int64)
    return (x >> 1) ^ -(x & 1)


def aux_of(v, interval, packed, dc):
    """the aux entries of one stream from its coded symbols v: (out uint64, prev uint16, state uint8, dc uint16) per checkpoint.
    runLengthDecode's machine, one symbol at a time: state 0 fresh, 1 value, 2 count."""
    v = [int(x) for x in v]
    out, prev, state, sums = [], [], [], []
    at, st, acc = 0, 0, 0
    for i, cur in enumerate(v):
        if i % interval == 0:
            out.append(at)
            prev.append(v[i - 1] if packed and i else 0)
            state.append(st if packed else 0)
            sums.append(acc & 0xFFFF if dc else 0)
        if packed and st == 2:
            symbol, copies, st = v[i - 1], cur, 0
        else:
            symbol, copies = cur, 1
            if packed:
                st = 2 if st == 1 and cur == v[i - 1] else 1
        at += copies
        if dc:
            acc += copies * int(zigzag(symbol))
    return (np.array(out, np.uint64), np.array(prev, np.uint16), np.array(state, np.uint8), np.array(sums, np.uint16))


@functools.lru_cache(maxsize=None)
def expected_aux(blob, interval):
    """[1 + 6K] per stream (the lengths stream first): None, or the four arrays of aux_of"""
    import imageexperiments_amd as ia
    s = ia.read_compressed(blob, coded=True)
    k = s["K"]
    interval = interval or DEFAULT_INTERVAL
    out = [None]
    for i, (codes, packed) in enumerate(zip(s["codes"], s["packed"])):
        dc = i % (2 * k) == 1
        out.append(aux_of(codes, interval, bool(packed), dc) if packed or dc else None)
    return out


def chunk_rule(out, r0, r1):
    """(c0, c1) of a stream with aux entries: the last checkpoint at or in front of r0, the first behind it at or behind r1"""
    n = len(out)
    if r0 >= r1 or n == 0:
        return 0, 0
    c0 = int(np.searchsorted(out, r0, side="right")) - 1
    behind = [j for j in range(c0 + 1, n) if int(out[j]) >= r1]
    return c0, behind[0] if behind else n


@functools.lru_cache(maxsize=None)
def expected_chunks(blob, interval, rect, version):
    """chunks[6K, 2] the windowed parse reads without "parse all" """
    import imageexperiments_amd as ia
    _, h, k, _ = ia.container_info(blob)
    s = ia.read_compressed(blob, coded=True)
    _, ranges = region_cases.expected_window(blob, rect, h)
    step = interval or DEFAULT_INTERVAL
    aux = expected_aux(blob, interval)
    chunks = np.zeros((6 * k, 2), np.uint64)
    for i in range(6 * k):
        n = -(-len(s["codes"][i]) // step)
        r0, r1 = int(ranges[i // 2, 0]), int(ranges[i // 2, 1])
        if aux[i + 1] is None:
            chunks[i] = (min(r0 // step, n), min(-(-r1 // step), n))
        elif version == 1:
            chunks[i] = (0, n)
        else:
            chunks[i] = chunk_rule(aux[i + 1][0], r0, r1)
    return chunks


def inside(blob, interval, rect):
    """[(i, c0, c1, entry state)] of the streams with aux entries whose chunk range is strictly inside: 0 < c0, c1 < n_chunks"""
    aux = expected_aux(blob, interval)
    chunks = expected_chunks(blob, interval, rect, 2)
    out = []
    for i in range(chunks.shape[0]):
        if aux[i + 1] is None:
            continue
        c0, c1 = int(chunks[i, 0]), int(chunks[i, 1])
        if 0 < c0 and c0 < c1 < len(aux[i + 1][0]):
            out.append((i, c0, c1, int(aux[i + 1][2][c0])))
    return out


def check_coverage(ia):
    """what F1 and F2 are there for, from the numpy restatement: a changed oracle frame fails here instead of testing nothing"""
    s1 = ia.read_compressed(f1(), coded=True)
    k = s1["K"]
    dc = [i % (2 * k) == 1 for i in range(6 * k)]
    assert sum(1 for p, d in zip(s1["packed"], dc) if p and not d) >= 20
    assert all(s1["packed"][i] for i in (1, 2 * k + 1, 4 * k + 1))
    for interval, floor in ((32, 18), (100, 15)):
        got = inside(f1(), interval, ACROSS_1024)
        packed_inside = [g for g in got if s1["packed"][g[0]] and not dc[g[0]]]
        assert len(packed_inside) >= floor, (interval, len(packed_inside))
        assert sum(1 for g in got if dc[g[0]]) == 3, interval
    assert {g[3] for g in inside(f1(), 32, ACROSS_1024)} == {0, 1, 2}
    s2 = ia.read_compressed(f2(), coded=True)
    k = s2["K"]
    assert [bool(s2["packed"][i]) for i in (1, 2 * k + 1, 4 * k + 1)] == [False, False, True]
    long_packed = [i for i in range(6 * k) if s2["packed"][i] and len(s2["codes"][i]) > 2048]
    assert len(long_packed) >= 6 and max(len(s2["codes"][i]) for i in long_packed) > 3 * 2048
    got = inside(f2(), F2_INTERVAL, F2_INNER)
    packed_inside = [g for g in got if s2["packed"][g[0]]]
    assert len(packed_inside) >= 7, len(packed_inside)
    unaligned = [g for g in packed_inside if g[1] * F2_INTERVAL > 2048 and (g[1] * F2_INTERVAL) % 2048 != 0]
    assert len(unaligned) >= 4, len(unaligned)                      # the entry inside a block that is not the stream's first
    assert {1, 2 * k + 1} <= {g[0] for g in got}                    # both unpacked step-0 streams


def aux_section(index_v2, index_v1):
    """(offset, bytes) of a version-2 blob's aux section: it lies behind the version-1 part"""
    return len(index_v1), len(index_v2) - len(index_v1)


def aux_entry_offset(ia, index_v2, index_v1, stream, j):
    """byte offset in the version-2 blob of entry j of `stream` (1 ... 6K)"""
    info = ia.index_info(index_v1)
    k = info["K"]
    at = len(index_v1) + 8
    for s in range(1, stream):
        if info["streams"][s]["packed"] or (s - 1) % (2 * k) == 1:
            at += 16 * len(info["streams"][s]["checkpoints"])
    return at + 16 * j


def flip(blob, bit):
    a = bytearray(blob)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def damaged_aux(ia, index_v2, index_v1, seed, count=48):
    """[(what, bytes)]: single-bit flips confined to the aux section"""
    at, size = aux_section(index_v2, index_v1)
    rng = np.random.default_rng([20250309, seed])
    return [(f"aux flip of bit {pos}", flip(index_v2, 8 * at + int(pos))) for pos in rng.integers(0, 8 * size, count)]


def exit_flips(ia, blob, index_v2, index_v1, interval, rect):
    """[(what, bytes)]: for a few streams strictly inside, one flipped bit in out, prev, state and dc of entry c1"""
    s = ia.read_compressed(blob, coded=True)
    k = s["K"]
    out = []
    got = inside(blob, interval, rect)
    picked = [g for g in got if g[0] % (2 * k) == 1][:2] + [g for g in got if s["packed"][g[0]] and g[0] % (2 * k) != 1][:3]
    for i, c0, c1, _ in picked:
        at = 8 * aux_entry_offset(ia, index_v2, index_v1, i + 1, c1)
        fields = [("out", at + 0), ("out", at + 3), ("state", at + 64 + 32)]
        if s["packed"][i]:
            fields += [("prev", at + 64 + 0), ("prev", at + 64 + 9), ("state", at + 64 + 33)]
        if i % (2 * k) == 1:
            fields += [("dc", at + 64 + 16), ("dc", at + 64 + 27)]
        out += [(f"stream {i} entry {c1} {name} bit {bit - at}", flip(index_v2, bit)) for name, bit in fields]
    return out


def flip_in_chunk(ia, blob, v1, stream, chunk):
    """the container with the middle bit of chunk `chunk` of stream `stream` (1 ... 6K) flipped; positions come from the index"""
    s = ia.index_info(v1)["streams"][stream]
    cp = [int(c) for c in s["checkpoints"]] + [int(s["end_bit"])]
    return flip(blob, 8 * ((cp[chunk] + cp[chunk + 1]) // 2 // 8) + 7 - (cp[chunk] + cp[chunk + 1]) // 2 % 8)


def never_read_containers(ia, v1):
    """[(what, damaged container)]: F1 with a bit flipped in a chunk outside [c0, c1) of a packed and of a step-0 stream"""
    blob = f1()
    s = ia.read_compressed(blob, coded=True)
    k = s["K"]
    got = inside(blob, 32, ACROSS_1024)
    packed = [g for g in got if s["packed"][g[0]] and g[0] % (2 * k) != 1][0]
    dc = [g for g in got if g[0] % (2 * k) == 1][0]
    out = []
    for i, c0, c1, _ in (packed, dc):
        out.append((f"stream {i} chunk {c0 - 1} (in front)", flip_in_chunk(ia, blob, v1, i + 1, c0 - 1)))
        out.append((f"stream {i} chunk {c1} (behind)", flip_in_chunk(ia, blob, v1, i + 1, c1)))
    return out


def damaged_v2(ia, oracle, v1, v2):
    """parse_cases.damaged_indexes over F1's version-2 index (the other index: another frame's of the same geometry), plus
    flips confined to the aux section"""
    other_blob = bytes(oracle.OracleContext(region_cases.K, 8, region_cases.QUALITY).encode_image(
        oracle.synth_frame(region_cases.W, region_cases.H, 778)))
    other = ia.container_index(other_blob, 32, expanded=True)
    return parse_cases.damaged_indexes(v2, other, 2) + damaged_aux(ia, v2, v1, 0)
