"""The inputs and the expected values of the delta encoder's tests, shared by the host tests and the device tests (nothing here needs a
GPU).

The delta encoder keeps the last frame and pursues only the tiles whose pixels changed.  Three kernels stand around the unchanged tile
encoder, and this module is their model in numpy:
  changed_tiles  tile t = tx * tiles_y + ty is changed iff a pixel byte inside the image differs; the list is ascending
  pack           the listed tiles side by side in a frame of R x C whole tiles, black outside the image and in the padding tiles
  scatter        the packed frame's records j to tile list[j] of the whole frame's records
A frame lies in memory as a Layout: pixel (x, y) is the 3 bytes at raw[off + y * stride + 3 * x], with random bytes everywhere else --
in front, between the rows and behind -- so that a kernel that reads anything but pixels gives itself away.  `WRONG_DIFFS` and
`WRONG_PACKS` are the mistakes the cases must be able to tell from the model (tests/test_delta_cases.py checks that they can)."""
import functools

import numpy as np

QUALITY = 3.5
PACK_ROWS = 64                                  # MPC_DELTA_PACK_ROWS
# name: (width, height, K).  ragged: 11 x 6 tiles, ragged on both axes; full: K = 32 with the all-ones table, full-length records;
# many: 25 x 17 = 425 tiles, 7 packed columns
SHAPES = {"ragged": (83, 45, 8), "one": (8, 8, 8), "tiny": (5, 3, 8), "full": (16, 16, 32), "many": (200, 136, 8)}
STRIDES = ("tight", "odd", "word")


def quant(name):
    """the quantiser table a shape is encoded with: None = the context's at QUALITY; the all-ones "max" table for `full`"""
    return np.ones((3, SHAPES[name][2])) if name == "full" else None


def grid(w, h):
    return -(-w // 8), -(-h // 8)


def stride_of(kind, w):
    """tight; odd: the byte path; word: a multiple of 8 with padding (the word path where the base is aligned and 3 * w is a multiple of 8)"""
    return {"tight": 3 * w, "odd": 3 * w + 5, "word": (3 * w + 7) // 8 * 8 + 8}[kind]


@functools.lru_cache(maxsize=None)
def frame(w, h, seed):
    """gradient plus noise: tiles that are neither flat nor alike, so that counts are not trivial"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 127 // max(w + h - 2, 1)], axis=2)
    out = np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def bump(px, x, y, c=0):
    """a copy with byte c of pixel (x, y) moved by one"""
    out = np.array(px)
    out[y, x, c] ^= 1
    return out


def tile_pixel(t, w, h, rng=None):
    """a pixel of tile t inside the image: its top-left one, or a random one"""
    tx, ty = divmod(int(t), grid(w, h)[1])
    x1, y1 = min(tx * 8 + 8, w), min(ty * 8 + 8, h)
    return (tx * 8, ty * 8) if rng is None else (int(rng.integers(tx * 8, x1)), int(rng.integers(ty * 8, y1)))


def change_tiles(px, tiles, seed=0):
    """a copy in which exactly the listed tiles differ, each in one byte of one random pixel, by one"""
    rng = np.random.default_rng(seed)
    out = np.array(px)
    h, w = px.shape[:2]
    for t in tiles:
        x, y = tile_pixel(t, w, h, rng)
        out[y, x, int(rng.integers(0, 3))] ^= 1
    return out


class Layout:
    """a frame in memory: raw (uint8, 1-D), the first pixel at raw[off], `stride` bytes between rows; 8 rows of room behind the last row
    and 32 bytes behind those, so that even a reader of the out-of-image rows of a ragged tile stays inside `raw`"""

    def __init__(self, px, kind="tight", lead=0, seed=1):
        self.h, self.w = px.shape[:2]
        self.stride, self.off, self.kind = stride_of(kind, self.w), lead, kind
        self.raw = np.random.default_rng(seed).integers(0, 256, lead + (self.h + 8) * self.stride + 32, dtype=np.uint8)
        self.pixels[:] = px

    @property
    def pixels(self):
        """the h x w x 3 view of the pixels"""
        return np.lib.stride_tricks.as_strided(self.raw[self.off:], (self.h, self.w, 3), (self.stride, 3, 1))

    def rows(self, n_rows, n_bytes):
        """raw[off + y * stride + b] for y < n_rows, b < n_bytes: the memory as a reader of more than the pixels meets it"""
        return np.lib.stride_tricks.as_strided(self.raw[self.off:], (n_rows, n_bytes), (self.stride, 1))


# ---- the model ----
def pack_geometry(n, rows=PACK_ROWS):
    """(R, C, stride, bytes) of the packed frame of n listed tiles"""
    if n < 1:
        return 0, 0, 0, 0
    R = min(n, rows)
    C = -(-n // R)
    return R, C, 24 * C, 24 * C * 8 * R


def _list(flags_yx, order="ascending"):
    """[tiles_y, tiles_x] flags -> the list"""
    if order == "transposed":
        return np.flatnonzero(flags_yx.reshape(-1)).astype(np.int32)             # t = ty * tiles_x + tx
    t = np.flatnonzero(flags_yx.T.reshape(-1)).astype(np.int32)                 # t = tx * tiles_y + ty
    return t[::-1].copy() if order == "descending" else t


def changed_tiles(prev, cur):
    """the model: prev, cur h x w x 3 pixel arrays (any strides)"""
    h, w = cur.shape[:2]
    tx, ty = grid(w, h)
    differs = np.zeros((ty * 8, tx * 8), bool)
    differs[:h, :w] = (np.asarray(prev) != np.asarray(cur)).any(axis=2)
    return _list(differs.reshape(ty, 8, tx, 8).any(axis=(1, 3)))


def wrong_changed_tiles(a, b, mistake):
    """a diff with one mistake in it, on two Layouts of the same geometry"""
    h, w, stride = b.h, b.w, b.stride
    tx, ty = grid(w, h)
    n_bytes = max(24 * tx, stride)
    differs = a.rows(8 * ty, n_bytes) != b.rows(8 * ty, n_bytes)                 # every byte a careless reader could meet
    y, xb = np.mgrid[0:8 * ty, 0:n_bytes]
    inside = (y < h) & (xb < 3 * w)
    look = {"compares stride padding": (y < h) & (xb < stride),
            "compares the out-of-image columns and rows": xb < 24 * tx,
            "ignores the blue byte": inside & (xb % 3 != 2),
            "ignores the last image row": inside & (y < h - 1),
            "ignores the last image column": inside & (xb < 3 * (w - 1))}.get(mistake, inside)
    hit = differs & look
    flags = np.zeros((ty, tx), bool)
    for col in range(tx):                                                        # bytes behind the last tile column count for it
        hi = n_bytes if col == tx - 1 else 24 * col + 24
        flags[:, col] = hit[:, 24 * col:hi].reshape(ty, 8, -1).any(axis=(1, 2))
    return _list(flags, {"tx / ty transposed": "transposed", "list not ascending": "descending"}.get(mistake, "ascending"))


WRONG_DIFFS = ("compares stride padding", "compares the out-of-image columns and rows", "ignores the blue byte", "ignores the last image row",
               "ignores the last image column", "tx / ty transposed", "list not ascending")


def pack(px, tiles, rows=PACK_ROWS, mistake=None):
    """the model: the packed frame [8R, 8C, 3] of the listed tiles of the h x w x 3 pixels; an entry outside the frame's tiles is black"""
    h, w = px.shape[:2]
    tx, ty = grid(w, h)
    R, C, _, _ = pack_geometry(len(tiles), rows)
    out = np.full((8 * R, 8 * C, 3), 255 if mistake == "padding tiles not black" else 0, np.uint8)
    for j, t in enumerate(tiles):
        tile = np.zeros((8, 8, 3), np.uint8)
        if 0 <= t < tx * ty:
            cx, cy = divmod(int(t), ty)
            if mistake == "ragged tile not black-filled":                       # the edge pixels repeated, as a clamped fetch gives them
                tile = np.asarray(px)[np.minimum(np.arange(8) + cy * 8, h - 1)][:, np.minimum(np.arange(8) + cx * 8, w - 1)]
            else:
                src = np.asarray(px)[cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8]
                tile[:src.shape[0], :src.shape[1]] = src
        out[(j % R) * 8:(j % R) * 8 + 8, (j // R) * 8:(j // R) * 8 + 8] = tile
    return out


WRONG_PACKS = ("padding tiles not black", "ragged tile not black-filled")


def scatter(packed_counts, packed_choices, tiles, counts, choices):
    """the model: records j ([n, 3] counts, [n, 3, K] records) to tile tiles[j] of copies of the whole frame's; -> (counts, choices,
    an entry was outside the frame)"""
    counts, choices, bad = np.array(counts), np.array(choices), False
    for j, t in enumerate(tiles):
        if 0 <= t < counts.shape[0]:
            counts[t], choices[t] = packed_counts[j], packed_choices[j]
        else:
            bad = True
    return counts, choices, bad


# ---- the cases ----
def tile_sets(name):
    """{label: tiles}: the changed-tile sets a shape is tried with"""
    w, h, _ = SHAPES[name]
    tx, ty = grid(w, h)
    tiles = tx * ty
    rng = np.random.default_rng(tiles)
    sets = {"none": [], "first": [0], "last": [tiles - 1], "all": list(range(tiles)),
            "checkerboard": [cx * ty + cy for cx in range(tx) for cy in range(ty) if (cx + cy) % 2 == 0],
            "random": sorted(rng.choice(tiles, max(tiles // 3, 1), replace=False).tolist())}
    if tiles > 2:
        sets["interior"] = [(tx // 2) * ty + ty // 2]
        sets["all but one"] = [t for t in range(tiles) if t != tiles // 2]
    if tiles > PACK_ROWS + 1:
        sets["64"] = sorted(rng.choice(tiles, PACK_ROWS, replace=False).tolist())
        sets["65"] = sorted(rng.choice(tiles, PACK_ROWS + 1, replace=False).tolist())
    return sets


def diff_pairs(name, lead=0):
    """[(label, Layout before, Layout after)] for the diff: every stride kind with every tile set, and the changes a careless diff
    misses or invents.  The bytes that are no pixels differ between the two layouts of every pair.  lead: bytes in front (a device
    window at byte offset 1)"""
    w, h, _ = SHAPES[name]
    px = frame(w, h, 11)
    out = []
    for s, kind in enumerate(STRIDES):
        for label, tiles in tile_sets(name).items():
            out.append((f"{kind} {label}", Layout(px, kind, lead, 100 + s), Layout(change_tiles(px, tiles, s), kind, lead, 200 + s)))
        out.append((f"{kind} blue", Layout(px, kind, lead, 100 + s), Layout(bump(px, w // 2, h // 2, 2), kind, lead, 200 + s)))
        out.append((f"{kind} corner", Layout(px, kind, lead, 100 + s), Layout(bump(px, w - 1, h - 1, s), kind, lead, 200 + s)))
        if h > 1:
            out.append((f"{kind} last row", Layout(px, kind, lead, 100 + s), Layout(bump(px, 0, h - 1, 1), kind, lead, 200 + s)))
        if w > 1:
            out.append((f"{kind} last column", Layout(px, kind, lead, 100 + s), Layout(bump(px, w - 1, 0, 1), kind, lead, 200 + s)))
    return out


def expected(before, after):
    return changed_tiles(before.pixels, after.pixels)


def pack_cases(name):
    """[(label, pixels, tiles, rows)]: rows in {1, 3, 64} with n in {1, rows, rows + 1} where the frame has that many tiles, the tile
    sets, and a list that is not sorted"""
    w, h, _ = SHAPES[name]
    px = frame(w, h, 11)
    tiles = grid(w, h)[0] * grid(w, h)[1]
    rng = np.random.default_rng(7)
    out = []
    for rows in (1, 3, PACK_ROWS):
        for n in sorted({1, rows, rows + 1}):
            if n <= tiles:
                last = [tiles - 1] if n > 1 or tiles == 1 else []                # the ragged corner tile among them
                out.append((f"rows {rows} n {n}", px, sorted(rng.choice(tiles - 1, n - len(last), replace=False).tolist()) + last, rows))
    for label, listed in tile_sets(name).items():
        if listed:
            out.append((label, px, listed, PACK_ROWS))
    out.append(("unsorted", px, list(rng.permutation(tiles)[:max(tiles // 2, 1)]), 3))
    return out


def records(n, K, seed):
    """n tiles of hand-made records: counts [n, 3] in 0 ... K, records [n, 3, K] u32, zero beyond a count"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, K + 1, (n, 3)).astype(np.uint16)
    choices = rng.integers(1, 2**32, (n, 3, K), dtype=np.uint64).astype(np.uint32)
    choices[np.arange(K)[None, None, :] >= counts[:, :, None]] = 0
    return counts, choices


def sequence(name, steps=6, seed=3):
    """a frame sequence for a session: the first frame, then frames that each differ from the one before in a random set of tiles
    (none, one, a third, ...), deterministic"""
    w, h, _ = SHAPES[name]
    sets = list(tile_sets(name).values())
    frames = [np.array(frame(w, h, seed))]
    for i in range(steps - 1):
        frames.append(change_tiles(frames[-1], sets[(i * 5 + 1) % len(sets)], seed + i))
    return frames
