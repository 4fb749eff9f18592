"""Frame layouts for the tile encoders (mpc_encode_tiles_device, mpc_encode_batch_device, mpc_encode_tiles), shared by the GPU
tests (test_gpu_frame_layouts.py) and the CPU check of the cases themselves (test_layout_cases.py).

A LAYOUT places one or more tight frames inside a larger byte buffer: frame f, row y, pixel x, component c lives at byte
    offset + f * frame_stride + y * row_stride + 3 * x + c
of the parent.  `embed` builds that parent with every byte that is not a pixel set by a POISON; the expected records are always
the oracle's on the tight frames, so a kernel that reads one byte of padding, or one pixel through the wrong stride, differs.

The pursuit kernel's refill has two pixel fetches (mp_pursuit.hip): six 8-byte loads per lane when the launch's flag is set
(`flag_reasons` below restates mpcodec_context.cpp's three-alignment predicate) and every tile the wave takes is whole (`whole`),
and a clamped byte-by-byte fetch otherwise.  Every case names the branch it is there for; test_layout_cases.py proves the claim.

Tiles are queued tx outer, ty inner within the tile rows [a, b) of a frame, frame after frame (`queue_whole`): consecutive queue
entries are what one wave takes in one refill."""
from collections import namedtuple

import numpy as np

Layout = namedtuple("Layout", "offset row_stride frame_stride frames W H")
# offset: where frame 0 starts relative to an 8-byte aligned point of the parent (embed adds a margin that is a multiple of 8);
# frame_stride: 0 for a single frame passed without one.

Case = namedtuple("Case", "name layout K seed stripes claims")
# stripes: tile row ranges [a, b) the case runs besides the full height; claims: what test_layout_cases.py proves about it.

POISONS = ("zero", "random")
MARGIN_EXTRA = 64                    # the parent exceeds the view by at least one row stride and this many bytes, on both sides


def tiles_of(layout):
    return (layout.W + 7) // 8, (layout.H + 7) // 8


def span(layout):
    """bytes from the first pixel byte of frame 0 to the last pixel byte of the last frame, inclusive"""
    return (layout.frames - 1) * layout.frame_stride + (layout.H - 1) * layout.row_stride + 3 * layout.W


def margin(layout):
    """front and back margin of the parent: at least one row stride and MARGIN_EXTRA bytes, a multiple of 8"""
    return (layout.row_stride + MARGIN_EXTRA + 7) // 8 * 8


def pixel_index(layout):
    """byte offsets, relative to frame 0's first byte, of every pixel byte: int64 [frames, H, W, 3]"""
    f = np.arange(layout.frames, dtype=np.int64)[:, None, None, None] * layout.frame_stride
    y = np.arange(layout.H, dtype=np.int64)[None, :, None, None] * layout.row_stride
    x = np.arange(layout.W, dtype=np.int64)[None, None, :, None] * 3
    c = np.arange(3, dtype=np.int64)[None, None, None, :]
    return f + y + x + c


def _neighbours(buf, is_pixel):
    """for every byte the value of the nearest pixel byte before it and after it in memory (-1 where there is none)"""
    n = buf.size
    at = np.arange(n)
    before = np.maximum.accumulate(np.where(is_pixel, at, -1))
    after = np.minimum.accumulate(np.where(is_pixel, at, n)[::-1])[::-1]
    prev = np.where(before >= 0, buf[np.maximum(before, 0)].astype(np.int16), -1)
    nxt = np.where(after < n, buf[np.minimum(after, n - 1)].astype(np.int16), -1)
    return prev, nxt


def embed(frames, layout, poison):
    """frames: uint8 [frames, H, W, 3] (or [H, W, 3] for one) -> (parent uint8 [n], byte offset of frame 0 in it).
    poison "zero": every non-pixel byte 0x00; "random": a seeded fill of non-zero bytes, none equal to the nearest pixel byte
    before or after it in memory (a read that slips by one byte cannot return the right value by accident)."""
    frames = np.ascontiguousarray(frames, np.uint8).reshape(layout.frames, layout.H, layout.W, 3)
    if poison not in POISONS:
        raise ValueError(poison)
    start = margin(layout) + layout.offset
    n = start + span(layout) + margin(layout)
    at = start + pixel_index(layout)
    is_pixel = np.zeros(n, bool)
    is_pixel[at.reshape(-1)] = True
    assert int(is_pixel.sum()) == frames.size, "the layout's pixels overlap"
    if poison == "zero":
        parent = np.zeros(n, np.uint8)
        parent[at.reshape(-1)] = frames.reshape(-1)
        return parent, start
    rng = np.random.default_rng(0x5EED + 31 * layout.row_stride + layout.offset + 7 * layout.frames)
    parent = rng.integers(1, 256, n).astype(np.uint8)
    parent[at.reshape(-1)] = frames.reshape(-1)
    prev, nxt = _neighbours(parent, is_pixel)
    bad = ~is_pixel & ((parent == prev) | (parent == nxt))
    for c in (1, 2, 3):                                  # three non-zero candidates, at most two of them excluded
        fix = bad & (prev != c) & (nxt != c)
        parent[fix] = c
        bad &= ~fix
    assert not bad.any()
    return parent, start


def extract(parent, start, layout):
    """the tight frames back out of a parent: uint8 [frames, H, W, 3]"""
    return parent[start + pixel_index(layout)]


def host_view(parent, start, layout, frame=0):
    """frame `frame` as a [H, W, 3] numpy view ON the parent (strides (row_stride, 3, 1)): no copy"""
    return np.ndarray((layout.H, layout.W, 3), np.uint8, buffer=parent, offset=start + frame * layout.frame_stride,
                      strides=(layout.row_stride, 3, 1))


# ---- the kernel's predicates, restated --------------------------------------------------------------------------------

def flag_reasons(layout, base_mod8=0):
    """Why the launch's 8-byte flag is CLEAR: the subset of {"pointer", "row_stride", "frame_stride"} whose alignment fails
    (empty = the flag is set).  mpcodec_context.cpp: rgb % 8 == 0 && row_stride % 8 == 0 && (frames <= 1 || frame_stride % 8 == 0).
    base_mod8: the parent's own address mod 8 (device and staging allocations are 256-byte aligned: 0)."""
    why = set()
    if (base_mod8 + margin(layout) + layout.offset) % 8:
        why.add("pointer")
    if layout.row_stride % 8:
        why.add("row_stride")
    if layout.frames > 1 and layout.frame_stride % 8:
        why.add("frame_stride")
    return why


def flag_set(layout, base_mod8=0):
    return not flag_reasons(layout, base_mod8)


def whole(tx, ty, W, H):
    """the refill's per-tile predicate: all 64 pixels of tile (tx, ty) lie inside the image"""
    return tx * 8 + 8 <= W and ty * 8 + 8 <= H


def queue_whole(layout, a=0, b=None):
    """`whole` of every tile in queue order: frames outer, then tx, then ty in [a, b)"""
    tiles_x, tiles_y = tiles_of(layout)
    b = tiles_y if b is None else b
    one = [whole(tx, ty, layout.W, layout.H) for tx in range(tiles_x) for ty in range(a, b)]
    return np.array(one * layout.frames, bool)


def longest_run(mask):
    best = cur = 0
    for m in mask:
        cur = cur + 1 if m else 0
        best = max(best, cur)
    return best


# ---- the cases ------------------------------------------------------------------------------------------------------------

def _single(name, W, H, row_stride, offset=0, K=8, seed=0, stripes=(), **claims):
    return Case(name, Layout(offset, row_stride, 0, 1, W, H), K, seed, tuple(stripes), claims)


def _batch(name, frames, W, H, row_stride, frame_stride, K=8, seed=0, stripes=(), **claims):
    return Case(name, Layout(0, row_stride, frame_stride, frames, W, H), K, seed, tuple(stripes), claims)


PARENT_W, PARENT_H = 96, 64          # the image the crop cases are windows of (row_stride 288)


def _crops():
    out = []
    for (W, H) in ((40, 24), (41, 27)):
        for (x0, y0) in ((8, 8), (5, 3), (PARENT_W - W, PARENT_H - H)):
            off = y0 * 3 * PARENT_W + 3 * x0
            out.append(_single(f"crop-{W}x{H}-at-{x0}-{y0}", W, H, 3 * PARENT_W, offset=off, seed=300 + x0 + W,
                               flag=(3 * x0) % 8 == 0, clear_by=() if (3 * x0) % 8 == 0 else ("pointer",), window=(x0, y0)))
    return out


CASES = [
    # 8-byte path, padded rows, all tiles whole
    _single("pad8", 64, 48, 3 * 64 + 8, seed=101, flag=True, clear_by=(), all_whole=True),
    # 8-byte path on five whole columns of 50 tiles, byte path on the ragged sixth, same launch; stripes with a > 0
    _single("pad8-ragged-x", 44, 400, 136, seed=102, stripes=((17, 41), (40, 50)), flag=True, clear_by=(), whole_run=32, edge_tiles=True),
    # flag set, short columns: waves mixing whole and edge tiles
    _single("pad8-ragged-xy", 70, 50, 216, seed=103, flag=True, clear_by=(), edge_tiles=True, ragged_x=True, ragged_y=True),
    # byte path on a width that is a multiple of 8
    _single("pad-odd", 64, 48, 3 * 64 + 5, seed=104, flag=False, clear_by=("row_stride",), all_whole=True),
    # byte path chosen by the pointer alone
    _single("offset-odd-1", 64, 48, 192, offset=1, seed=105, flag=False, clear_by=("pointer",), all_whole=True),
    _single("offset-odd-3", 64, 48, 192, offset=3, seed=106, flag=False, clear_by=("pointer",), all_whole=True),
    _single("offset-odd-4", 64, 48, 192, offset=4, seed=107, flag=False, clear_by=("pointer",), all_whole=True),
] + _crops() + [
    # tile 0 not whole while the flag is set (lanes that take nothing evaluate tile 0), and its whole counterpart
    _single("narrow-3x5", 3, 5, 64, seed=108, flag=True, clear_by=(), tile0_whole=False),
    _single("narrow-8x8", 8, 8, 64, seed=109, flag=True, clear_by=(), tile0_whole=True, all_whole=True),
    # a batch through both fetches with a gap between frames; stripes, one ending in the ragged last tile row
    _batch("batch-pad", 4, 70, 50, 216, 216 * 50 + 40, seed=110, stripes=((2, 5), (4, 7)), flag=True, clear_by=(), edge_tiles=True,
           ragged_y=True, frame_gap=40),
    # frame_stride % 8 != 0 alone clears the flag for frames > 1
    _batch("batch-odd", 3, 64, 48, 192, 3 * 64 * 48 + 3, seed=111, flag=False, clear_by=("frame_stride",), all_whole=True),
    # ragged width in a batch, tight
    _batch("batch-ragged", 4, 139, 100, 3 * 139, 3 * 139 * 100, seed=112, flag=False, clear_by=("row_stride", "frame_stride"),
           ragged_x=True, ragged_y=True, tight=True),
    # the other end of K, once
    _single("K32", 44, 400, 136, K=32, seed=113, flag=True, clear_by=(), whole_run=32, edge_tiles=True),
]

BY_NAME = {c.name: c for c in CASES}
STEPS_PATH_CASES = ("pad8-ragged-xy", "pad-odd", "batch-pad")       # run again under MPC_PATH=steps (mp_init_kernel's own addressing)


def case_frames(case, synth_frame):
    """the case's tight frames, uint8 [frames, H, W, 3]; synth_frame: the oracle's generator"""
    L = case.layout
    return np.stack([synth_frame(L.W, L.H, 1000 * case.seed + f) for f in range(L.frames)])


def stripe_of(arrays, frames, tiles_x, tiles_y, a, b):
    """whole-frame oracle outputs of `frames` frames (each array [frames * tiles_x * tiles_y, ...], tile = tx * tiles_y + ty) ->
    the entries of tile rows [a, b) in the encoders' output order, tile = frame * tiles_x * (b - a) + tx * (b - a) + (ty - a)"""
    out = []
    for arr in arrays:
        v = arr.reshape((frames, tiles_x, tiles_y) + arr.shape[1:])[:, :, a:b]
        out.append(np.ascontiguousarray(v).reshape((frames * tiles_x * (b - a),) + arr.shape[1:]))
    return tuple(out)
