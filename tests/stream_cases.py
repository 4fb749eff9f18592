"""Symbol streams that exercise every branch of the entropy stage (CompressedImage.cpp:359-460, Huffman.cpp:246-279):
runs cut at 0x8001 symbols, runs across the device's 4096-symbol blocks, the `packed + 4 < size` boundary, empty and
one-symbol streams, symbols up to 0xFFFF, Huffman ties in every order of first appearance, Golomb-friendly streams.

K = 4 on a 2048x1536 frame (49 152 tiles): 24 code streams of up to 1 179 648 symbols in all, 147 456 lengths.
`as_coded`: what the encoder's stream assembly hands the entropy stage (step-0 coefficient streams already differenced);
`as_held`: the same with those three streams undifferenced (what writeCompressed / the oracle take)."""
import numpy as np

W, H, K, BS = 2048, 1536, 4, 8
TILES = (W // 8) * (H // 8)
CHUNK = 0x8001


def _zigzag(d):
    d = d.astype(np.int64)
    return ((d << 1) ^ (d >> 63)).astype(np.uint64)


def _dc_difference(v):
    v = v.astype(np.int64)
    prev = np.concatenate([[0], v[:-1]])
    return (_zigzag(v - prev) & 0xFFFF).astype(np.uint16)


def make():
    rng = np.random.default_rng(20241004)
    u16 = lambda a: np.asarray(a, dtype=np.uint16)                                    # noqa: E731
    geometric = lambda p, n: u16(np.minimum(rng.geometric(p, n) - 1, 65535))         # noqa: E731
    runs = lambda lens, vals: u16(np.repeat(vals, lens))                              # noqa: E731
    held = [
        u16([]),                                                                       # 0 empty
        u16([5]),                                                                      # 1 (DC slot) one symbol
        u16(np.zeros(100000)),                                                         # 2 three full chunks + a rest
        u16(np.full(CHUNK, 7)),                                                        # 3 exactly one chunk
        u16(np.full(CHUNK + 1, 7)),                                                    # 4 chunk + 1
        u16(np.full(CHUNK + 2, 9)),                                                    # 5 chunk + 2
        geometric(0.3, 60000),                                                         # 6 small alphabet
        u16(rng.integers(0, 65536, 20000)),                                            # 7 symbols beyond the LDS bins
        runs(rng.integers(1, 11, 9000), rng.integers(0, 4, 9000)),                     # 8 short runs (adjacent runs may merge)
        u16(np.cumsum(rng.integers(-3, 4, 40000)) + 1000),                             # 9 (DC slot, 2K+1) random walk
        runs([4095, 4097, 8192, 1, 4096, 4096, 3], [1, 2, 3, 4, 5, 5, 6]),             # 10 runs against the 4096-symbol blocks
        runs(np.full(5000, 3), rng.integers(0, 50, 5000)),                             # 11 runs of three
        u16(rng.integers(0, 8192, 50000)),                                             # 12 a large flat alphabet
        u16(np.concatenate([np.zeros(CHUNK - 1), [1]])),                               # 13 one symbol short of a chunk
        u16(np.concatenate([np.zeros(2 * CHUNK), [1, 1]])),                            # 14 two chunks exactly, then a pair
        runs(np.full(3000, 2), np.arange(3000) % 7),                                   # 15 pairs: run lengths make it longer
        u16(np.full(7, 3)),                                                            # 16 packed + 4 == size: not shorter
        u16(np.concatenate([np.cumsum(rng.integers(-1, 2, 5000)) + 300, np.full(70000, 123)])),   # 17 (DC slot, 4K+1) walk, then flat
        u16(np.full(50000, 0xFFFF)),                                                   # 18 the largest symbol, in runs
        u16(np.arange(30000)),                                                         # 19 all distinct, ascending
        u16(np.arange(30000)[::-1]),                                                   # 20 all distinct, descending
        u16(np.tile(rng.permutation(64), 200)),                                        # 21 64 symbols, equal counts: all ties
        u16(np.minimum(rng.geometric(0.004, 30000) - 1, 4000)),                        # 22 wide geometric: large Golomb M
        u16(np.concatenate([np.full(8, 3), rng.integers(0, 3, 4096 * 3 - 8), np.full(2 * CHUNK + 5, 2), [1]])),   # 23 mixture
    ]
    assert len(held) == 6 * K
    coded = list(held)
    for i in (1, 2 * K + 1, 4 * K + 1):
        coded[i] = _dc_difference(held[i])
    counts = u16(rng.integers(0, K + 1, 3 * TILES))
    assert sum(len(x) for x in coded) <= 2 * 3 * TILES * K
    return dict(W=W, H=H, K=K, bs=BS, counts=counts, as_coded=coded, as_held=held)


def quant(K):
    return np.arange(1, 3 * K + 1, dtype=np.float64).reshape(3, K) * 3


# ---- the stream fuzzer's cases (tools/fuzz_streams.py, tests/test_gpu_fuzz_slice.py) -------------------------------------

def random_stream(rng, cap):
    kind = int(rng.integers(0, 8))
    n = int(rng.integers(0, cap + 1)) if rng.random() < 0.9 else 0
    if n == 0:
        return np.zeros(0, np.uint16)
    if kind == 0:
        return np.minimum(rng.geometric(rng.uniform(0.02, 0.9), n) - 1, 65535).astype(np.uint16)
    if kind == 1:
        return rng.integers(0, int(rng.choice([2, 16, 300, 9000, 65536])), n).astype(np.uint16)
    if kind == 2:                                                   # runs of random lengths, some beyond the 0x8001 cut
        out = []
        while sum(len(x) for x in out) < n:
            length = int(rng.choice([1, 2, 3, 7, 8, 4095, 4096, 4097, 0x8000, 0x8001, 0x8002, 70000])) if rng.random() < 0.5 else int(rng.integers(1, 40))
            out.append(np.full(length, rng.integers(0, int(rng.choice([3, 70000])) % 65536 + 1), np.uint16))
        return np.concatenate(out)[:n]
    if kind == 3:
        return np.full(n, rng.integers(0, 65536), np.uint16)
    if kind == 4:
        return (np.arange(n) % int(rng.integers(1, 70000))).astype(np.uint16)
    if kind == 5:                                                   # equal counts: every Huffman tie there is
        k = int(rng.integers(1, 300))
        return np.tile(rng.permutation(k), n // k + 1)[:n].astype(np.uint16)
    if kind == 6:
        return np.repeat(rng.integers(0, 5, n // 2 + 1), 2)[:n].astype(np.uint16)
    return (np.cumsum(rng.integers(-2, 3, n)) % 1000).astype(np.uint16)


def fuzz_streams(rng, cases):
    """Yields dict(K, W, H, counts, as_held, as_coded, quant): 6K random streams per case (K = 1..6, frames of 64..199 x 64..119
    tiles) within the capacity of the frame's records.  rng: a seed or a numpy Generator."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    for _ in range(cases):
        K = int(rng.integers(1, 7))
        W, H = 8 * int(rng.integers(8, 200)), 8 * int(rng.integers(8, 120))
        tiles = (W // 8) * (H // 8)
        cap = 2 * 3 * tiles * K
        held, left = [], cap
        for _ in range(6 * K):
            s = random_stream(rng, min(left, max(1, cap // (3 * K))))
            left -= len(s)
            held.append(s)
        coded = list(held)
        for i in (1, 2 * K + 1, 4 * K + 1):
            coded[i] = _dc_difference(held[i]) if len(held[i]) else held[i]
        counts = rng.integers(0, K + 1, 3 * tiles).astype(np.uint16)
        yield dict(K=K, W=W, H=H, counts=counts, as_held=held, as_coded=coded, quant=quant(K))
