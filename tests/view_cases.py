"""The inputs and the expected values of the view tests, shared by the host tests and the device tests (nothing here needs a GPU).

A view is a rectangle of a frame, reconstructed from the first `steps` records of every tile-channel and reduced by 2^scale_log2.
Its expected pixels are the ORACLE's decode of the container truncated with the oracle's own reader and writer, cropped and reduced
here in numpy as include/mpcodec.h defines the reduction; its expected parse is region_cases.expected_window of that container."""
import functools

import numpy as np

import region_cases

STEPS = (0, 1, 2, 3, 8, 9)                      # of the main input (K = 8): all, three cuts, K, above K
SCALES = (0, 1, 2, 3)
WHOLE = (0, 0, 0, 0)
RECTS = (
    region_cases.ACROSS_1024,                   # tiles 988 ... 1026: two gather blocks
    (256, 0, 5, 277),                           # the ragged last tile column, top to bottom
    (0, 272, 261, 5),                           # the ragged last tile row
    (232, 144, 5, 4),                           # inside one tile, cells cut on the right and below
    (8, 8, 1, 1),
    (0, 0, region_cases.W, region_cases.H),
)
UNALIGNED = (233, 147, 5, 4)
PARSE_STEPS = (1, 2, 3, 8, 0)
PARSE_RECTS = (WHOLE, region_cases.ACROSS_1024, (256, 0, 5, 277))
SMALL_W, SMALL_H, SMALL_K, SMALL_QUALITY = 40, 24, 32, 3.5
SMALL_STEPS = (0, 1, 5, 31, 32, 40)


def main():
    """261x277, K = 8, ragged in both directions, packed streams, lengths 0 ... 8"""
    return region_cases.container()


@functools.lru_cache(maxsize=None)
def small():
    """40x24 at K = 32 from the oracle"""
    from oracle import oracle_py as oracle
    return bytes(oracle.OracleContext(SMALL_K, 8, SMALL_QUALITY).encode_image(oracle.synth_frame(SMALL_W, SMALL_H, 4024)))


def kept(blob_k, steps):
    """the steps a view keeps: 0 = all, above K acts as K"""
    return blob_k if steps <= 0 or steps > blob_k else steps


@functools.lru_cache(maxsize=None)
def truncated(blob, steps):
    """the container cut to `steps` >= 1 steps by the oracle: lengths min(length, steps), streams of later steps empty"""
    from oracle import oracle_py as oracle
    st = oracle.read_compressed(blob)
    k = st["K"]
    st["lengths"] = np.minimum(st["lengths"], steps).astype(np.uint16)
    for i in range(6 * k):
        if (i % (2 * k)) // 2 >= steps:
            st["codes"][i] = np.zeros(0, np.uint16)
    return oracle.write_compressed(st)


@functools.lru_cache(maxsize=None)
def _decoded(blob, steps, fast):
    from oracle import oracle_py as oracle
    cut = blob if steps == 0 else truncated(blob, steps)
    return (oracle.decode_image_fast if fast else oracle.decode_image)(cut)


def resolve(rect, width, height):
    return (0, 0, width, height) if tuple(rect) == WHOLE else tuple(rect)


def reduce(pixels, scale_log2):
    """output pixel (i, j) = (sum + n // 2) // n over the n pixels of its c x c cell that exist, per colour channel, in integers"""
    c = 1 << scale_log2
    h, w, _ = pixels.shape
    oh, ow = -(-h // c), -(-w // c)
    padded = np.zeros((oh * c, ow * c, 3), np.int64)
    padded[:h, :w] = pixels
    there = np.zeros((oh * c, ow * c), np.int64)
    there[:h, :w] = 1
    sums = padded.reshape(oh, c, ow, c, 3).sum(axis=(1, 3))
    n = there.reshape(oh, c, ow, c).sum(axis=(1, 3))[..., None]
    assert n.min() >= 1 and n.max() <= c * c
    return ((sums + n // 2) // n).astype(np.uint8)


def expected_view(blob, view, fast=False):
    """the pixels of view = (rect, steps, scale_log2): the oracle's decode of the truncation, cropped, reduced"""
    rect, steps, scale_log2 = view
    full = _decoded(blob, steps, fast)
    x, y, w, h = resolve(rect, full.shape[1], full.shape[0])
    return reduce(full[y:y + h, x:x + w], scale_log2)


def expected_parse(blob, rect, steps, k):
    """(symbols, ranges) of the view's parse: the windowed parse of the truncated container"""
    import imageexperiments_amd as ia
    w, h, _, _ = ia.container_info(blob)
    cut = blob if steps == 0 or steps >= k else truncated(blob, steps)
    return region_cases.expected_window(cut, resolve(rect, w, h), h)


def flip_in_stream(blob, index, stream):
    """one bit flipped in the middle of the payload of stream `stream` of the 1 + 6K: between its first checkpoint and its end"""
    import imageexperiments_amd as ia
    s = ia.index_info(index)["streams"][stream]
    assert len(s["checkpoints"]) >= 1 and s["end_bit"] > s["checkpoints"][0] + 8
    bit = (int(s["checkpoints"][0]) + int(s["end_bit"])) // 2
    a = bytearray(blob)
    a[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(a)


def zigzag(v):
    return (v << 1) ^ (v >> 31)


def dictionary_case(ia, discriminating=True):
    """An 8x8 container at K = 8 whose luma record is base 0, then a detail row, then base 5.  Base 0's block holds rows
    510 ... 572 of the dynamic dictionary; row 573 is the first row of the block that only base choice 5 -- step 2 -- unlocks.  With
    that row as choice 1 the first two steps alone are not decodable, the first one and all three are."""
    k = 8
    second = 510 + 63 if discriminating else 510
    lengths = np.array([3, 0, 0], np.uint16)
    codes = [np.zeros(0, np.uint16) for _ in range(6 * k)]
    for step, delta in enumerate((0, zigzag(second), zigzag(5 - second))):
        codes[2 * step] = np.array([delta], np.uint16)
        codes[2 * step + 1] = np.array([zigzag(5)], np.uint16)
    return ia.write_compressed(8, 8, k, 8, np.full((3, k), 16.0), lengths, codes)
