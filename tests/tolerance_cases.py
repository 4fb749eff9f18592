"""The delta encoder's change tolerance as a numpy model, with the cases the host definition and the kernel are held to (nothing here
needs a GPU; include/mpcodec.h, "delta with a change tolerance").

  sse(t)     the sum of (cur - kept)^2 over the pixel bytes of tile t inside the image
  changed    sse(t) > T;   held: 0 < sse(t) <= T
  composite  cur in the changed tiles, kept -- whole -- in every other

`diff` is that definition on two delta_cases.Layouts; with a `mistake` it is the definition with one thing wrong (WRONG), and
tests/test_tolerance_cases.py checks that the cases tell every one of them from the model.  The shapes cross the kernel's own seams: a
workgroup takes a strip of 64 tiles of one tile row and the flags -> list kernels take 1024 tiles a block, and delta_cases.SHAPES never
leaves one strip or one block."""
import functools

import numpy as np

import delta_cases as dc

# name: (width, height).  ragged2: 67 x 4 tiles, two strips, the last tile row 5 pixel rows, 3 * width odd (the byte path); word2: 66
# tiles across, tight stride 1584 (the 8-byte path); blocks: 130 x 9 = 1170 tiles, three strips, two list blocks
SHAPES = {"one": (8, 8), "tiny": (5, 3), "ragged2": (531, 29), "word2": (528, 32), "blocks": (1040, 72)}
STRIDES = dc.STRIDES
K = 8
MAX_SSE = 64 * 3 * 255 * 255
assert MAX_SSE == 12484800

WRONG = (">= instead of >", "threshold per chunk column", "threshold per channel", "kept copy updated for held tiles",
         "kept copy updated chunk-wise where bytes differ", "stride padding counted", "out-of-image columns and rows counted",
         "byte difference wrapped modulo 256", "absolute instead of squared difference", "blue byte ignored", "16-bit accumulation",
         "neighbour of a changed tile overwritten")


def grid(name):
    return dc.grid(*SHAPES[name])


# ---- the model ----
def diff(a, b, T, mistake=None):
    """kept Layout a, current Layout b (the same geometry and stride) -> (list int32 ascending, sse uint32 [tiles], composite h x w x 3)"""
    h, w, stride = b.h, b.w, b.stride
    assert (a.h, a.w, a.stride) == (h, w, stride)
    tx, ty = dc.grid(w, h)
    n_bytes = max(24 * tx, stride)
    A, B = a.rows(8 * ty, n_bytes).astype(np.int64), b.rows(8 * ty, n_bytes).astype(np.int64)
    d = B - A
    if mistake == "byte difference wrapped modulo 256":
        d = d & 255
    e = np.abs(d) if mistake == "absolute instead of squared difference" else d * d
    y, xb = np.mgrid[0:8 * ty, 0:n_bytes]
    inside = (y < h) & (xb < 3 * w)
    look = {"stride padding counted": (y < h) & (xb < stride), "out-of-image columns and rows counted": xb < 24 * tx,
            "blue byte ignored": inside & (xb % 3 != 2)}.get(mistake, inside)
    e = e * look
    col = np.arange(n_bytes)
    chunk_of, tile_of = np.minimum(col // 8, 3 * tx - 1), np.minimum(col // 24, tx - 1)   # bytes behind the last tile column count for it
    by_chunk, by_channel = np.zeros((3 * tx, 8 * ty), np.int64), np.zeros((3 * tx, 8 * ty), np.int64)
    np.add.at(by_chunk, chunk_of, e.T)
    np.add.at(by_channel, 3 * tile_of + col % 3, e.T)
    by_chunk = by_chunk.T.reshape(ty, 8, tx, 3).sum(axis=1)                               # [ty, tx, 3]
    by_channel = by_channel.T.reshape(ty, 8, tx, 3).sum(axis=1)
    sse = by_chunk.sum(axis=2)
    if mistake == "16-bit accumulation":
        sse = sse & 0xffff
    if mistake == ">= instead of >":
        changed = sse >= T
    elif mistake == "threshold per chunk column":
        changed = (by_chunk > T).any(axis=2)
    elif mistake == "threshold per channel":
        changed = (by_channel > T).any(axis=2)
    else:
        changed = sse > T
    kept, cur = np.array(a.pixels), np.array(b.pixels)
    write = changed
    if mistake == "kept copy updated for held tiles":
        write = sse > 0
    elif mistake == "neighbour of a changed tile overwritten":
        write = changed.copy()
        write[1:] |= changed[:-1]
        write[:-1] |= changed[1:]
        write[:, 1:] |= changed[:, :-1]
        write[:, :-1] |= changed[:, 1:]
    composite = kept.copy()
    for cy, cx in zip(*np.nonzero(write)):
        composite[cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = cur[cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8]
    if mistake == "kept copy updated chunk-wise where bytes differ":                      # the write rule of the diff without a tolerance
        rows_k, rows_c = composite.reshape(h, 3 * w), cur.reshape(h, 3 * w)
        for c0 in range(0, 3 * w, 8):
            moved = (rows_k[:, c0:c0 + 8] != rows_c[:, c0:c0 + 8]).any(axis=1)
            rows_k[moved, c0:c0 + 8] = rows_c[moved, c0:c0 + 8]
    return dc._list(changed), sse.T.reshape(-1).astype(np.uint32), composite


def diff_pixels(kept, cur, T):
    """the model on two pixel arrays"""
    return diff(dc.Layout(kept, "tight", 0, 1), dc.Layout(cur, "tight", 0, 2), T)


def held_totals(sse, T):
    held = (sse > 0) & (sse <= T)
    return int(held.sum()), int(sse[held].astype(np.uint64).sum())


# ---- the tile cases ----
@functools.lru_cache(maxsize=None)
def scene(name, seed=11):
    """a frame with every byte in 64 ... 191: room to move either way"""
    w, h = SHAPES[name]
    out = (dc.frame(w, h, seed) // 2 + 64).astype(np.uint8)
    out.setflags(write=False)
    return out


def tile_box(name, t):
    """the in-image part of tile t: (x0, y0, pixel columns, pixel rows)"""
    w, h = SHAPES[name]
    cx, cy = divmod(int(t), grid(name)[1])
    return cx * 8, cy * 8, min(8, w - cx * 8), min(8, h - cy * 8)


def add_bytes(px, name, t, moves):
    """in place: byte b of in-image row r of tile t moved by v, for (r, b, v) in moves; negative r and b count from the tile's in-image end"""
    x0, y0, pw, ph = tile_box(name, t)
    for r, b, v in moves:
        r, b = r % ph, b % (3 * pw)
        px[y0 + r].reshape(-1)[3 * x0 + b] += v


def spread(px, name, t, values, rng):
    """in place: tile t gets sum(v^2 for v in values) of sse, on distinct random in-image bytes of it"""
    x0, y0, pw, ph = tile_box(name, t)
    where = rng.choice(ph * 3 * pw, len(values), replace=False)
    add_bytes(px, name, t, [(int(p) // (3 * pw), int(p) % (3 * pw), v) for p, v in zip(where, values)])


def marks(name):
    """the tiles at the kernel's seams: the first and last tile of every strip in the first and last tile row, the tiles round a list
    block's end, tile 0 and the last tile"""
    tx, ty = grid(name)
    out = {0, tx * ty - 1}
    for cx in (0, 63, 64, 127, 128, tx - 1):
        for cy in (0, ty - 1):
            if cx < tx:
                out.add(cx * ty + cy)
    out.update(t for t in (1023, 1024) if t < tx * ty)
    return sorted(out)


def tile_cases(name, kind, lead=0):
    """[(label, kept Layout, current Layout, T)].  The bytes that are no pixels differ between the two layouts of every pair."""
    w, h = SHAPES[name]
    tx, ty = grid(name)
    tiles = tx * ty
    base = scene(name)
    rng = np.random.default_rng(tiles + len(kind))
    out = []

    def case(label, cur, T, kept=base):
        cur = np.asarray(cur)
        assert cur.min() >= 0 and cur.max() <= 255
        out.append((f"{kind} {label}", dc.Layout(kept, kind, lead, 100 + len(out)), dc.Layout(cur.astype(np.uint8), kind, lead, 200 + len(out)), T))

    # sse exactly T (held) and T + 1 (changed) on the seam tiles, either way round: 49 + 1 = 50, 49 + 1 + 1 = 51
    for flip in (0, 1):
        cur = np.array(base, np.int64)
        for i, t in enumerate(marks(name)):
            spread(cur, name, t, (7, -1) if (i + flip) % 2 == 0 else (7, -1, 1), rng)
        case(f"exact {flip}", cur, 50)
    # the whole difference in one chunk column: 100 + 1 on bytes of one 8-byte column of every third tile
    cur = np.array(base, np.int64)
    for i, t in enumerate(range(0, tiles, 3)):
        pw = tile_box(name, t)[2]
        c0 = 8 * (i % 3) if 8 * (i % 3) + 1 < 3 * pw else 0
        add_bytes(cur, name, t, [(i, c0, 10), (i + 1, c0 + 1, -1)])
    case("one column", cur, 100)
    # spread: 49 in each of three bytes of three channels -- and, where the tile is 8 pixels wide, of three chunk columns: no column and
    # no channel exceeds 100, the tile (147) does
    cur = np.array(base, np.int64)
    for t in range(0, tiles, 2):
        pw = tile_box(name, t)[2]
        add_bytes(cur, name, t, [(0, 0, 7), (-1, 3 * (pw // 2) + 1, -7), (t, 3 * pw - 1, 7)])
    case("spread", cur, 100)
    # only the last in-image row or column of the tiles on the image's edges: 16 > 10 in the corner, 9 <= 10 along the edges
    cur = np.array(base, np.int64)
    for cx in range(tx):
        add_bytes(cur, name, cx * ty + ty - 1, [(-1, cx, 4 if cx == tx - 1 else 3)])
    for cy in range(ty - 1):
        add_bytes(cur, name, (tx - 1) * ty + cy, [(cy, -1, 3)])
    case("last row and column", cur, 10)
    # cur < kept and cur > kept on the same bytes: 5 * 9 = 45
    for sign in (1, -1):
        for T in (45, 44):
            cur = np.array(base, np.int64)
            for t in range(0, tiles, 2):
                add_bytes(cur, name, t, [(j, 4 * j, 3 * sign) for j in range(5)])
            case(f"sign {sign:+d} T {T}", cur, T)
    # 0 against 255 everywhere: 12 484 800 in every whole tile, one below it and at it
    lo, hi = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    case("0 to 255 below", hi, MAX_SSE - 1, lo)
    case("0 to 255 at", hi, MAX_SSE, lo)
    case("255 to 0 below", lo, MAX_SSE - 1, hi)
    # T = 0: a byte by one in a third of the tiles; T = 2^32 - 1: another frame altogether
    case("T 0", dc.change_tiles(base, list(range(0, tiles, 3)), 5), 0)
    case("T max", scene(name, 12), 2**32 - 1)
    # a changed tile (101) whose neighbours are held (100 each), at an interior tile and at the seams
    cur = np.array(base, np.int64)
    centres = sorted({(min(cx, tx - 1), min(cy, ty - 1)) for cx in (1, 63, 64, tx - 2) for cy in (1, ty - 2) if cx >= 0 and cy >= 0})
    taken = set()
    for cx, cy in centres:
        cross = [(cx, cy)] + [(cx + dx, cy + dy) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)) if 0 <= cx + dx < tx and 0 <= cy + dy < ty]
        if taken & set(cross):
            continue
        taken |= set(cross)
        for i, (x, y) in enumerate(cross):
            spread(cur, name, x * ty + y, (10, 1) if i == 0 else (10,), rng)
    case("cross", cur, 100)
    # noise everywhere, -2 ... 2: about 384 a whole tile, held and changed side by side
    noise = rng.integers(-2, 3, (h, w, 3))
    case("noise", base + noise, 384)
    return out


# ---- sequences ----
def noise_sequence(name, frames=7, seed=5):
    """a fixed scene under fresh uniform noise of -2 ... 2 in every frame (none in the last tile column, so that its tiles stay byte for
    byte what was sent), a bright 8 x 8 block that moves a tile per frame, and frame 4 a repeat of frame 3 -> (frames, T)"""
    w, h = SHAPES[name]
    tx, ty = grid(name)
    rng = np.random.default_rng(seed)
    base = scene(name, 21).astype(np.int64)
    out = []
    for i in range(frames):
        if i == 4:
            out.append(out[-1].copy())
            continue
        px = base + rng.integers(-2, 3, (h, w, 3))
        px[:, 8 * (tx - 1):] = base[:, 8 * (tx - 1):]
        cx, cy = (2 + i) % max(tx - 1, 1), min(1, ty - 1)
        px[8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] += 60
        out.append(px.astype(np.uint8))
    return out, 800                     # two noises apart: 192 * 2 * 2 = 768 a whole tile on average


def ramp_sequence(name, frames=8):
    """one whole tile gains 1 in every byte every frame: 192 j^2 after j frames, so at T = 1000 it is sent at j = 3 (1728) and the count
    starts again from the pixels sent -> (frames, T, the tile)"""
    w, h = SHAPES[name]
    tx, ty = grid(name)
    cx, cy = min(64, tx - 1), min(1, ty - 1)
    assert tile_box(name, cx * ty + cy)[2:] == (8, 8)
    base = np.array(scene(name, 31))
    out = []
    for i in range(frames):
        px = base.copy()
        px[8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] += i
        out.append(px)
    return out, 1000, cx * ty + cy


SEQUENCES = {"noise ragged2": lambda: noise_sequence("ragged2")[:2] + ("ragged2",), "noise blocks": lambda: noise_sequence("blocks")[:2] + ("blocks",),
             "ramp word2": lambda: ramp_sequence("word2")[:2] + ("word2",), "ramp ragged2": lambda: ramp_sequence("ragged2")[:2] + ("ragged2",)}


@functools.lru_cache(maxsize=None)
def sequence(label):
    """-> (frames, T, shape name)"""
    return SEQUENCES[label]()


def replay(frames, tolerances, mistake=None):
    """a session over the frames, call i at tolerance tolerances[i] (or one value for all) -> per call dict(key, list, sse, composite,
    held, held_sse); the first call is the key frame"""
    if np.isscalar(tolerances):
        tolerances = [tolerances] * len(frames)
    h, w = frames[0].shape[:2]
    tiles = dc.grid(w, h)[0] * dc.grid(w, h)[1]
    out, comp = [], None
    for px, T in zip(frames, tolerances):
        if comp is None:
            comp = np.array(px)
            out.append(dict(key=1, list=np.arange(tiles, dtype=np.int32), sse=None, composite=comp, held=0, held_sse=0))
            continue
        lst, sse, comp = diff(dc.Layout(comp, "tight", 0, 1), dc.Layout(px, "tight", 0, 2), T, mistake)
        held, held_sse = held_totals(sse, T)
        out.append(dict(key=0, list=lst, sse=sse, composite=comp, held=held, held_sse=held_sse))
    return out
