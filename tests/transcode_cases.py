"""The inputs and the expected values of the transcode tests, shared by the host tests and the device tests (nothing here needs a
GPU).

A transcode is a view of a container as a container: the records of a tile-aligned rectangle's tiles, cut to the first `steps` steps,
in the new frame's tile order, coded again.  `model` is that definition in numpy over read_compressed / write_compressed; for a
container an encoder made from pixels the result is the encoder's own container of the cropped pixels, truncated (`fresh`)."""
import functools

import numpy as np

import region_cases
import view_cases

WHOLE = view_cases.WHOLE
W, H, K = region_cases.W, region_cases.H, region_cases.K
# tile aligned in the 261x277 frame; a ragged right or bottom edge only where it is the frame's own
RECTS = (
    (0, 0, W, H),                               # the whole frame: the source container itself
    (224, 64, 37, 24),                          # columns 28 ... 32 (ragged, the frame's edge), rows 8 - 10: across tile 1024
    (40, 64, 168, 96),                          # interior, through the flat band and the checkerboard: packed streams
    (256, 272, 5, 5),                           # the ragged corner tile
    (96, 0, 80, 277),                           # the flat band, top to bottom
    (0, 0, 8, 8),                               # the first tile
    (176, 40, 40, 160),                         # the checkerboard
)
INTERIOR = (40, 64, 168, 96)
STEPS = (0, 1, 3, 8, 9)                         # all, two cuts, K, above K
# (rect, steps, scale_log2) that are MPC_ERR_ARGUMENT on the 261x277 frame
ARGUMENT_ERRORS = (
    ((4, 0, 8, 8), 0, 0),                       # x not aligned
    ((0, 3, 8, 8), 0, 0),                       # y not aligned
    ((0, 0, 12, 8), 0, 0),                      # a right edge that is neither aligned nor the frame's
    ((0, 0, 8, 13), 0, 0),                      # a bottom edge likewise
    ((8, 8, 250, 8), 0, 0),                     # right edge at 258: inside the ragged column, not the frame's 261
    ((0, 0, 8, 8), 0, 1),                       # scale_log2 != 0
    ((0, 0, 8, 8), 0, -1),
    (WHOLE, 0, 2),
    ((0, 0, 8, 8), -1, 0),                      # steps < 0
    ((0, 0, 0, 8), 0, 0),                       # empty
    ((0, 0, 8, 0), 0, 0),
    ((0, 8, 0, 0), 0, 0),                       # not "the whole frame": that is (0, 0, 0, 0)
    ((0, 0, W + 3, 8), 0, 0),                   # outside
    ((256, 0, 8, 8), 0, 0),
    ((W + 3, 0, 8, 8), 0, 0),
    ((0, 272, 8, 8), 0, 0),
    ((-8, 0, 16, 8), 0, 0),
    ((0, 0, 2**31 - 1, 8), 0, 0),               # x + width would overflow
    ((8, 8, 2**31 - 8, 2**31 - 8), 0, 0),
)
BS4 = (30, 22, 5, 4, 3.5)                       # width, height, K, block size, quality of the block-size-4 frame
BS4_RECT = (8, 4, 22, 12)


def resolve(rect, width, height):
    return view_cases.resolve(rect or WHOLE, width, height)


def aligned(rect, width, height, bs):
    x, y, w, h = rect
    inside = w >= 1 and h >= 1 and 0 <= x and 0 <= y and x + w <= width and y + h <= height
    return inside and x % bs == 0 and y % bs == 0 and ((x + w) % bs == 0 or x + w == width) and ((y + h) % bs == 0 or y + h == height)


def records(streams):
    """(counts[tiles, 3], [per (channel, step): position of every tile's record in that stream pair, -1 = none])"""
    k = streams["K"]
    counts = np.asarray(streams["lengths"], np.int64).reshape(-1, 3)
    assert counts.max(initial=0) <= k
    places = []
    for ch in range(3):
        for step in range(k):
            live = counts[:, ch] > step
            places.append(np.where(live, np.cumsum(live) - 1, -1))
    return counts, places


def model(blob, view):
    """the definition: read_compressed -> records -> the rectangle's tiles in the new order, cut -> streams -> write_compressed.
    Raises MpcError for what read_compressed refuses, ValueError for a length above K"""
    import imageexperiments_amd as ia
    rect, steps, scale_log2 = view
    assert scale_log2 == 0 and steps >= 0
    s = ia.read_compressed(blob)
    k, bs = s["K"], s["bs"]
    if np.asarray(s["lengths"]).max(initial=0) > k:
        raise ValueError("a length above K")
    m = k if steps == 0 or steps > k else steps
    x, y, w, h = resolve(rect, s["W"], s["H"])
    assert aligned((x, y, w, h), s["W"], s["H"], bs)
    tiles_y = -(-s["H"] // bs)
    tx0, tx1, ty0, ty1 = x // bs, -(-(x + w) // bs), y // bs, -(-(y + h) // bs)
    # the new frame's tiles in its own order, t' = (tx - tx0) * nty + (ty - ty0), as tiles of the source
    source = (np.arange(tx0, tx1)[:, None] * tiles_y + np.arange(ty0, ty1)[None, :]).reshape(-1)
    counts, places = records(s)
    lengths = np.minimum(counts[source], m).astype(np.uint16)
    codes = []
    for ch in range(3):
        for step in range(k):
            at = places[ch * k + step][source]
            at = at[at >= 0] if step < m else at[:0]
            for half in (0, 1):
                codes.append(np.asarray(s["codes"][2 * (ch * k + step) + half], np.uint16)[at])
    return ia.write_compressed(w, h, k, bs, s["quant"].astype(np.float64), lengths.reshape(-1), codes)


@functools.lru_cache(maxsize=None)
def _encoded(rect):
    from oracle import oracle_py as oracle
    x, y, w, h = rect
    pixels = np.ascontiguousarray(region_cases.frame()[y:y + h, x:x + w])
    return bytes(oracle.OracleContext(K, 8, region_cases.QUALITY).encode_image(pixels))


def fresh(rect, steps):
    """the oracle's encode of the cropped pixels of region_cases.frame(), truncated by the oracle where steps cuts"""
    blob = _encoded(tuple(resolve(rect, W, H)))
    return blob if steps == 0 or steps >= K else view_cases.truncated(blob, steps)


@functools.lru_cache(maxsize=None)
def bs4():
    """(pixels, container) of the block-size-4 frame from the oracle"""
    from oracle import oracle_py as oracle
    w, h, k, bs, quality = BS4
    pixels = oracle.synth_frame(w, h, 3022).copy()
    return pixels, bytes(oracle.OracleContext(k, bs, quality).encode_image(pixels))
