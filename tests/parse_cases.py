"""Containers for the seek index's tests, shared by the host tests and the device tests (nothing here needs a GPU).

A - D are written by ia.write_compressed from chosen counts and contents, and are consistent: every stream has exactly the length
the lengths stream implies.  E (real) are oracle encodes.  check_coverage asserts, from index_info, what A - D are meant to
cover."""
import functools
import os

import numpy as np

from container_cases import FRAMES

INTERVALS = (32, 100, 4800, 65536)
EDGE_INTERVAL = 100


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return np.array(f[:n])


def _contents(kind, n, rng):
    if kind == 0:
        return rng.geometric(0.3, n)
    if kind == 1:
        return rng.integers(0, 65536, n)
    if kind == 2:                                                   # short runs of 4 symbols
        return np.repeat(rng.integers(0, 50, (n + 3) // 4), 4)[:n]
    if kind == 3:
        return np.full(n, 7)
    if kind == 4:                                                   # symbol k fib(k) times for 18 symbols, shuffled, as often as n asks
        pool = np.repeat(np.arange(18), _fib(18))
        return np.concatenate([rng.permutation(pool) for _ in range(n // pool.size + 1)])[:n]
    if kind == 5:
        return np.minimum(rng.geometric(0.004, n), 4000)
    if kind == 6:                                                   # 64 symbols with equal counts
        return rng.permutation(np.arange(n) % 64)
    return np.cumsum(rng.integers(-3, 4, n)) & 0xFFFF              # a random walk


def _write(ia, W, H, K, counts, contents):
    """counts[tiles, 3]; contents(i, n) -> the n symbols of stream i"""
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert counts.shape == (tiles, 3) and counts.max() <= K
    codes = []
    for i in range(6 * K):
        ch, step = (i // 2) // K, (i // 2) % K
        n = int((counts[:, ch] > step).sum())
        codes.append(np.asarray(contents(i, n), np.int64).astype(np.uint16))
        assert codes[-1].size == n
    return ia.write_compressed(W, H, K, 8, np.ones((3, K)), counts.astype(np.uint16).reshape(-1), codes)


def case_a(ia, seed=0):
    """640x480, K = 4: random counts, stream contents cycling through eight kinds"""
    rng = np.random.default_rng([20250301, seed])
    counts = rng.integers(0, 5, (4800, 3))
    return _write(ia, 640, 480, 4, counts, lambda i, n: _contents(i % 8, n, rng))


def case_b(ia, seed=0):
    """edge lengths for an interval of 100: channel 2's step streams hold 101, 100, 99 and 1 symbols, channel 1's steps 1 - 3 none"""
    rng = np.random.default_rng([20250302, seed])
    tiles = 300
    counts = np.zeros((tiles, 3), np.int64)
    counts[:, 0] = rng.integers(0, 5, tiles)
    counts[:, 1] = rng.integers(0, 2, tiles)
    counts[:, 2] = rng.permutation(np.array([4] + [3] * 98 + [2, 1] + [0] * (tiles - 101)))
    return _write(ia, 160, 120, 4, counts, lambda i, n: rng.integers(0, 65536, n))


def case_c(ia, seed=0):
    """1280x960, K = 1: stream 0 holds symbol k fib(k) times, k < 20, shuffled: 17 710 symbols, a Huffman table 20 bits deep"""
    rng = np.random.default_rng([20250303, seed])
    tiles = 19200
    counts = rng.integers(0, 2, (tiles, 3))
    counts[:, 0] = rng.permutation(np.arange(tiles) < 17710)
    skewed = rng.permutation(np.repeat(np.arange(20), _fib(20)))
    assert skewed.size == 17710
    return _write(ia, 1280, 960, 1, counts, lambda i, n: skewed if i == 0 else rng.geometric(0.3, n))


def case_d(ia, seed=0):
    """640x480, K = 1: stream 0 is Golomb coded with three outliers whose unary parts are some 240 bits long"""
    rng = np.random.default_rng([20250304, seed])
    tiles = 4800
    counts = rng.integers(0, 2, (tiles, 3))
    counts[:, 0] = rng.permutation(np.arange(tiles) < 2003)
    values = rng.permutation(np.concatenate([np.minimum(rng.geometric(0.004, 2000) - 1, 4000), [60000] * 3]))
    return _write(ia, 640, 480, 1, counts, lambda i, n: values if i == 0 else rng.geometric(0.3, n))


MAKERS = {"A": case_a, "B": case_b, "C": case_c, "D": case_d}


@functools.lru_cache(maxsize=None)
def synthetic(seed=0):
    """{name: container} of A - D"""
    import imageexperiments_amd as ia
    return {name: make(ia, seed) for name, make in MAKERS.items()}


@functools.lru_cache(maxsize=None)
def serial(blob):
    """the serial coded parse of a container as one array (the lengths stream, then the 6K coded streams), and the stream sizes"""
    import imageexperiments_amd as ia
    s = ia.read_compressed(blob, coded=True)
    parts = [s["lengths"]] + s["codes"]
    return np.concatenate(parts), [len(p) for p in parts]


def check_coverage(ia):
    """what A - D are there for, read from their indexes"""
    modes, packed, lengths, deep = set(), set(), set(), False
    blobs = synthetic()
    for name, blob in blobs.items():
        info = ia.index_info(ia.container_index(blob, EDGE_INTERVAL))
        for j, s in enumerate(info["streams"]):
            modes.add(s["mode"])
            lengths.add(s["n_coded"])
            if j:
                packed.add(s["packed"])
    assert modes == {0, 1} and packed == {False, True} and 0 in lengths
    # B: channel 2's four step streams (deltaId and coefficient each) around the interval, channel 1's later steps empty
    b = ia.index_info(ia.container_index(blobs["B"], EDGE_INTERVAL))["streams"]
    assert [b[1 + 2 * 4 * 2 + i]["n_coded"] for i in range(8)] == [101, 101, 100, 100, 99, 99, 1, 1]
    assert [len(b[1 + 2 * 4 * 2 + i]["checkpoints"]) for i in range(8)] == [2, 2, 1, 1, 1, 1, 1, 1]
    assert [b[1 + 2 * 4 * 1 + i]["n_coded"] for i in range(2, 8)] == [0] * 6
    assert not any(s["packed"] for s in b)
    # C: a Huffman table deeper than any 11-bit window (the stream coded on its own writes the same table: its first byte)
    c = ia.index_info(ia.container_index(blobs["C"], EDGE_INTERVAL))["streams"][1]
    stream0 = ia.read_compressed(blobs["C"], coded=True)["codes"][0]
    assert c["mode"] == 0 and c["n_coded"] == 17710 and not c["packed"] and ia.huffman_encode(stream0)[0] == 20
    # D: Golomb, with unary parts longer than any 64-bit window
    d = ia.index_info(ia.container_index(blobs["D"], EDGE_INTERVAL))["streams"][1]
    assert d["mode"] == 1 and d["n_coded"] == 2003 and 60000 // d["m"] > 64


SMALL_FRAMES = (0, 1, 2, 5, 6, 7, 8, 10)        # the containers of FRAMES below 100 000 bytes (container_cases.corpus)


def real(oracle, seed=100):
    """E: [(name, container)] of the small oracle encodes of container_cases.FRAMES (seed 100: the ones corpus() damages)"""
    out = []
    for n in SMALL_FRAMES:
        W, H, K, quality = FRAMES[n]
        octx = oracle.OracleContext(K, 8, 0.0 if quality == "max" else quality)
        out.append((f"E{n}", bytes(octx.encode_image(oracle.synth_frame(W, H, seed + n), quant=np.ones((3, K)) if quality == "max" else None))))
    return out


def golden_mn():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r0c1de5e1t_3_5.mn"), "rb") as f:
        return f.read()


def damaged_indexes(index, other, seed):
    """[(what, bytes)]: 64 single-bit flips anywhere in the index, 16 in its header, 16 truncations, and `other`: the index of
    another container of the same geometry"""
    a = np.frombuffer(index, np.uint8)
    rng = np.random.default_rng([20250305, seed])
    out = []
    for what, bits, count in (("flip", 8 * len(a), 64), ("header flip", 8 * 56, 16)):
        for pos in rng.integers(0, bits, count):
            c = a.copy()
            c[pos // 8] ^= 1 << (pos % 8)
            out.append((f"{what} of bit {pos}", bytes(c)))
    out += [(f"cut to {len(a) * k // 16}", bytes(a[:len(a) * k // 16])) for k in range(16)]
    out.append(("another container's", other))
    return out
