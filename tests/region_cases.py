"""The frame and the rectangles of the region decoder's tests, shared by the host tests and the device tests (nothing here needs a
GPU), and the expected values: slices of the serial parse, expanded and summed here in numpy."""
import functools

import numpy as np

W, H, K, QUALITY = 261, 277, 8, 3.5
TILES_X, TILES_Y = 33, 35                       # ragged in both directions; tile 1024 = column 29, row 9
INTERVALS = (32, 100, 0)
ACROSS_1024 = (224, 64, 16, 24)                 # columns 28 and 29, rows 8 - 10: tiles 988 ... 1026

RECTS = (
    (0, 0, W, H),
    (0, 0, 1, 1),
    (260, 276, 1, 1),
    ACROSS_1024,
    (5, 3, 50, 70),
    (100, 0, 3, 277),
    (0, 130, 261, 2),
    (256, 0, 5, 277),
    (120, 50, 20, 20),                          # inside the flat part
    (233, 147, 5, 4),                           # inside one tile
)


@functools.lru_cache(maxsize=None)
def frame():
    """synthetic detail, a flat band (long runs: packed streams) and a checkerboard"""
    from oracle import oracle_py as oracle
    rgb = oracle.synth_frame(W, H, 777).copy()
    assert rgb.shape == (H, W, 3)
    rgb[:, 96:176] = (90, 140, 200)
    v, u = np.mgrid[40:200, 176:216]
    rgb[40:200, 176:216] = np.where(((u // 8 + v // 8) % 2 == 0)[..., None], 30, 220).astype(np.uint8)
    return np.ascontiguousarray(rgb)


@functools.lru_cache(maxsize=None)
def container():
    """the frame encoded by the oracle on the CPU"""
    from oracle import oracle_py as oracle
    return bytes(oracle.OracleContext(K, 8, QUALITY).encode_image(frame()))


def tile_range(rect, height, bs=8):
    """(t0, t1, grid) of a rectangle in a frame of this height"""
    x, y, w, h = rect
    tiles_y = -(-height // bs)
    tx0, tx1, ty0, ty1 = x // bs, -(-(x + w) // bs), y // bs, -(-(y + h) // bs)
    return tx0 * tiles_y + ty0, (tx1 - 1) * tiles_y + ty1, (tx0, tx1, ty0, ty1)


def rle_expand(v):
    """runLengthDecode: a symbol that repeats the value in front of it is followed by a count of further copies"""
    out, state, prev = [], 0, None
    for cur in (int(x) for x in v):
        if state == 2:
            out.extend([prev] * cur)
            state = 0
        else:
            out.append(cur)
            state = 2 if state == 1 and cur == prev else 1
        prev = cur
    return np.array(out, np.uint16)


def dc_sum(v):
    """wrapping sums of the zig-zag decoded differences, low 16 bits"""
    x = v.astype(np.int64)
    return (np.cumsum((x >> 1) ^ -(x & 1)) & 0xFFFF).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def expanded(blob):
    """(lengths, [6K expanded streams], K) from the serial coded parse"""
    import imageexperiments_amd as ia
    s = ia.read_compressed(blob, coded=True)
    k = s["K"]
    out = []
    for i, (codes, packed) in enumerate(zip(s["codes"], s["packed"])):
        v = rle_expand(codes) if packed else np.asarray(codes, np.uint16)
        out.append(dc_sum(v) if i % (2 * k) == 1 else v)
    assert [len(v) for v in out] == list(s["expect"])
    return np.asarray(s["lengths"], np.uint16), out, k


def expected_window(blob, rect, height):
    """(symbols, ranges[3K, 2]) the windowed parse must give: counts of the lengths, slices of the expansion"""
    lengths, streams, k = expanded(blob)
    t0, t1, _ = tile_range(rect, height)
    counts = np.minimum(lengths.reshape(-1, 3).astype(np.int64), k)
    ranges = np.zeros((3 * k, 2), np.uint64)
    for ch in range(3):
        for step in range(k):
            ranges[ch * k + step] = ((counts[:t0, ch] > step).sum(), (counts[:t1, ch] > step).sum())
    parts = [lengths] + [streams[i][int(ranges[i // 2, 0]):int(ranges[i // 2, 1])] for i in range(6 * k)]
    return np.concatenate(parts), ranges


def check_coverage(ia):
    """what the frame is there for, read from its index at interval 32"""
    blob = container()
    assert ia.container_info(blob) == (W, H, K, 8) and (TILES_X, TILES_Y) == (-(-W // 8), -(-H // 8))
    streams = ia.index_info(ia.container_index(blob, 32))["streams"][1:]
    dc = [i % (2 * K) == 1 for i in range(6 * K)]
    packed = [s for s, d in zip(streams, dc) if s["packed"] and not d and len(s["checkpoints"]) >= 8]
    unpacked = [(i, s) for i, (s, d) in enumerate(zip(streams, dc)) if not s["packed"] and not d and len(s["checkpoints"]) >= 8]
    assert len(packed) >= 4 and len(unpacked) >= 4, (len(packed), len(unpacked))
    assert {s["mode"] for _, s in unpacked} == {0, 1}
    t0, t1, _ = tile_range(ACROSS_1024, H)
    assert t0 < 1024 < t1
    _, ranges = expected_window(blob, ACROSS_1024, H)
    inner = [i for i, s in unpacked
             if int(ranges[i // 2, 0]) // 32 > 0 and -(-int(ranges[i // 2, 1]) // 32) < len(s["checkpoints"]) and ranges[i // 2, 1] > ranges[i // 2, 0]]
    assert inner, "no unpacked stream whose window is strictly inside its chunks"


def crop(full, rect):
    x, y, w, h = rect
    return full[y:y + h, x:x + w]
