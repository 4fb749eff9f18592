"""The inputs and the expected values of the compose tests, shared by the host tests and the device tests (nothing here needs a GPU).

A compose is the inverse of a transcode: the container of a frame assembled from tile-aligned rectangles of containers.  A part is
(source, rect, x, y): rectangle `rect` of container `source` (None = all of it) lands at (x, y); parts are applied in order and a later
part wins a tile.  `model` is that definition in numpy over read_compressed / write_compressed; for containers an encoder made from
pixels with one quantiser table the result is the encoder's own container of the pasted pixels (`pasted`)."""
import functools

import numpy as np

import region_cases
import transcode_cases

WHOLE = None
W, H, K, QUALITY = region_cases.W, region_cases.H, region_cases.K, region_cases.QUALITY
CUT_X, CUT_Y = 128, 136                         # the quadrants' cut, tile aligned
EDITS = transcode_cases.RECTS[1:]               # the six non-whole rectangles; (224, 64, 37, 24) straddles tile 1024
MOVES = (
    ((40, 64, 168, 96), (8, 8)),                # interior to interior
    ((224, 64, 37, 24), (224, 128)),            # a ragged-edge rectangle to another place on the same ragged edge
    ((96, 0, 80, 277), (176, 0)),               # a full-height band: the ragged bottom stays the bottom
    ((0, 0, 8, 8), (248, 264)),                 # the first tile
    ((176, 40, 40, 160), (216, 112)),
)


@functools.lru_cache(maxsize=None)
def _frame(seed):
    from oracle import oracle_py as oracle
    return np.ascontiguousarray(oracle.synth_frame(W, H, seed).copy())


def _encode(pixels, quality=QUALITY, k=K, bs=8):
    from oracle import oracle_py as oracle
    return bytes(oracle.OracleContext(k, bs, quality).encode_image(np.ascontiguousarray(pixels)))


def frame():
    return region_cases.frame()


def container():
    return region_cases.container()


def other_frame():
    """a second frame of the same size"""
    return _frame(778)


@functools.lru_cache(maxsize=None)
def other_container():
    """... at the same quality: the same quantiser table"""
    return _encode(other_frame())


@functools.lru_cache(maxsize=None)
def other_quality_container():
    """a third at another quality: another quantiser table"""
    return _encode(_frame(779), 5.0)


@functools.lru_cache(maxsize=None)
def quadrants():
    """[(container of the quadrant, x, y)]: the four tile-aligned quadrants of the frame, cut by transcode_container"""
    import imageexperiments_amd as ia
    rects = ((0, 0, CUT_X, CUT_Y), (CUT_X, 0, W - CUT_X, CUT_Y), (0, CUT_Y, CUT_X, H - CUT_Y), (CUT_X, CUT_Y, W - CUT_X, H - CUT_Y))
    return tuple((ia.transcode_container(container(), (r, 0, 0)), r[0], r[1]) for r in rects)


@functools.lru_cache(maxsize=None)
def left_columns():
    """columns 0 ... 255 of the frame as a container"""
    import imageexperiments_amd as ia
    return ia.transcode_container(container(), ((0, 0, 256, H), 0, 0))


# the container-only part lists by name (lists() makes them)
NAMES = ("identity",) + tuple("edit %s" % (r,) for r in EDITS) + tuple("move %s to %s" % m for m in MOVES) + ("overlap", "quadrants", "side by side")
OVERLAP = ((1, (0, 0, 8, 8), 48, 72), (0, WHOLE, 0, 0), (1, (40, 64, 168, 96), 40, 64), (0, (40, 64, 168, 96), 8, 8))


@functools.lru_cache(maxsize=None)
def lists():
    """{name: (blobs, parts, width, height)}: every container-only part list of the tests"""
    main, other = container(), other_container()
    out = {"identity": ((main,), ((0, WHOLE, 0, 0),), W, H)}
    for rect in EDITS:
        out["edit %s" % (rect,)] = ((main, other), ((0, WHOLE, 0, 0), (1, rect, rect[0], rect[1])), W, H)
    for rect, (dx, dy) in MOVES:
        out["move %s to %s" % (rect, (dx, dy))] = ((main,), ((0, WHOLE, 0, 0), (0, rect, dx, dy)), W, H)
    out["overlap"] = ((main, other), OVERLAP, W, H)
    quads = quadrants()
    out["quadrants"] = (tuple(q[0] for q in quads), tuple((i, WHOLE, q[1], q[2]) for i, q in enumerate(quads)), W, H)
    out["side by side"] = ((left_columns(), main), ((0, WHOLE, 0, 0), (1, WHOLE, 256, 0)), 256 + W, H)
    assert tuple(out) == NAMES
    return out


def source_pixels(name):
    """the pixels every blob of lists()[name] was encoded from"""
    full, other = frame(), other_frame()
    if name == "quadrants":
        return tuple(full[y:y + (CUT_Y if y == 0 else H - CUT_Y), x:x + (CUT_X if x == 0 else W - CUT_X)] for _, x, y in quadrants())
    if name == "side by side":
        return (full[:, :256], full)
    return (full, other)[:len(lists()[name][0])]


def pasted(pixels, parts, width, height):
    """the pixels of the composition: parts' rectangles of `pixels[source]` (or the part's own array) pasted in order"""
    out = np.zeros((height, width, 3), np.uint8)
    for source, rect, dx, dy in parts:
        px = pixels[source] if isinstance(source, (int, np.integer)) else np.asarray(source)
        x, y, w, h = transcode_cases.resolve(rect, px.shape[1], px.shape[0])
        out[dy:dy + h, dx:dx + w] = px[y:y + h, x:x + w]
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's encode of the pasted pixels"""
    _, parts, width, height = lists()[name]
    return _encode(pasted(source_pixels(name), parts, width, height))


def edited(rect):
    """the frame with `rect` replaced by the other frame's pixels at the same place"""
    x, y, w, h = rect
    out = frame().copy()
    out[y:y + h, x:x + w] = other_frame()[y:y + h, x:x + w]
    return out


# (blobs as names, parts, width, height, a word of the text, "part N" / "source N" / None) that are MPC_ERR_ARGUMENT
ARGUMENT_ERRORS = (
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 8, 8), 4, 0)), W, H, "not aligned", "part 1"),            # misaligned x
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 8, 8), 0, 3)), W, H, "not aligned", "part 1"),            # misaligned y
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 12, 8), 0, 0)), W, H, "not aligned", "part 1"),           # a far edge neither aligned nor the frame's
    (("main",), ((0, WHOLE, 0, 0), (0, (4, 0, 8, 8), 0, 0)), W, H, "not aligned", "part 1"),            # the rectangle's own origin
    (("main",), ((0, WHOLE, 0, 0),), 2 * W, H, "ragged right edge", "part 0"),                          # 261 wide at x = 0 of a 522-wide frame
    (("main",), ((0, WHOLE, 0, 0),), W, 2 * H, "ragged bottom edge", "part 0"),
    (("main",), ((0, WHOLE, 0, 0), (0, (256, 0, 5, 8), 0, 0)), W, H, "ragged right edge", "part 1"),    # a ragged column moved inside
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 16, 8), 248, 0)), W, H, "not inside", "part 1"),          # hanging over the destination
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 8, 16), 0, 272)), W, H, "not inside", "part 1"),
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 8, 8), -8, 0)), W, H, "not aligned", "part 1"),
    (("main",), ((0, (0, 0, 256, H), 0, 0),), W, H, "tile 1120", None),                                 # column 32 uncovered
    (("main",), ((0, (8, 0, 253, H), 8, 0),), W, H, "tile 0 ", None),
    (("main",), ((0, WHOLE, 0, 0), (1, WHOLE, 0, 0)), W, H, "source 1 of 1", "part 1"),                 # a source out of range
    (("main",), ((0, WHOLE, 0, 0), (-2, WHOLE, 0, 0)), W, H, "source -2 of 1", "part 1"),
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 8, 8), 2**31 - 8, 0)), W, H, "not inside", "part 1"),     # x + w overflows an int
    (("main",), ((0, WHOLE, 0, 0), (0, (0, 0, 2**31 - 1, 8), 0, 0)), W, H, "not inside", "part 1"),
    (("main",), (), W, H, "n_parts", None),
    (("main",), ((0, WHOLE, 0, 0),), 0, H, "geometry", None),
    (("main", "other quality"), ((0, WHOLE, 0, 0),), W, H, "quantiser", "source 1"),                    # named by no part, still refused
    (("main", "bs4"), ((0, WHOLE, 0, 0),), W, H, "source 1: K", "source 1"),
)


@functools.lru_cache(maxsize=None)
def length_above_K():
    """the other container with one length of K raised to K + 1: the streams stay what the lengths, cut to K, promise"""
    import imageexperiments_amd as ia
    s = ia.read_compressed(other_container())
    lengths = s["lengths"].copy()
    lengths[int(np.flatnonzero(lengths == K)[0])] = K + 1
    return ia.write_compressed(s["W"], s["H"], s["K"], s["bs"], s["quant"].astype(np.float64), lengths, s["codes"])


def text_of(error):
    """an MpcError's text without its "mpcodec status N: " """
    return str(error).split(": ", 1)[1]


def named(name):
    return {"main": container, "other": other_container, "other quality": other_quality_container,
            "bs4": lambda: transcode_cases.bs4()[1]}[name]()


def records_of(blob):
    """(streams, counts[tiles, 3], records[tiles, 3, K, 2]) of a container; ValueError for a length above K"""
    import imageexperiments_amd as ia
    s = ia.read_compressed(blob)
    k = s["K"]
    if np.asarray(s["lengths"]).max(initial=0) > k:
        raise ValueError("a length above K")
    counts, places = transcode_cases.records(s)
    rec = np.zeros((counts.shape[0], 3, k, 2), np.uint16)
    for ch in range(3):
        for step in range(k):
            at = places[ch * k + step]
            live = at >= 0
            for half in (0, 1):
                rec[live, ch, step, half] = np.asarray(s["codes"][2 * (ch * k + step) + half], np.uint16)[at[live]]
    return s, counts, rec


def owners(blobs, parts, width, height):
    """owner[t] of every destination tile (-1 = uncovered), from the headers alone"""
    import imageexperiments_amd as ia
    bs = ia.container_info(blobs[0])[3]
    tiles_x, tiles_y = -(-width // bs), -(-height // bs)
    owner = -np.ones(tiles_x * tiles_y, np.int64)
    for p, (source, rect, dx, dy) in enumerate(parts):
        sw, sh = ia.container_info(blobs[source])[:2]
        x, y, w, h = transcode_cases.resolve(rect, sw, sh)
        ntx, nty = -(-(x + w) // bs) - x // bs, -(-(y + h) // bs) - y // bs
        dst = ((np.arange(ntx) + dx // bs)[:, None] * tiles_y + (np.arange(nty) + dy // bs)[None, :]).reshape(-1)
        owner[dst] = p
    return owner


def model(blobs, parts, width, height):
    """the definition: records of the owning parts placed in the destination's tile order -> streams -> write_compressed"""
    import imageexperiments_amd as ia
    owner = owners(blobs, parts, width, height)
    assert (owner >= 0).all()
    head = ia.read_compressed(blobs[0])
    k, bs = head["K"], head["bs"]
    tiles_y = -(-height // bs)
    parsed = {}
    counts = np.zeros((owner.size, 3), np.int64)
    rec = np.zeros((owner.size, 3, k, 2), np.uint16)
    for p, (source, rect, dx, dy) in enumerate(parts):
        mine = np.flatnonzero(owner == p)
        if not mine.size:
            continue                                                    # a part that owns nothing is not read
        if source not in parsed:
            parsed[source] = records_of(blobs[source])
        s, c, r = parsed[source]
        assert s["K"] == k and s["bs"] == bs
        x, y, w, h = transcode_cases.resolve(rect, s["W"], s["H"])
        assert transcode_cases.aligned((x, y, w, h), s["W"], s["H"], bs) and dx % bs == 0 and dy % bs == 0
        assert dx + w <= width and dy + h <= height
        assert (x + w) % bs == 0 or dx + w == width
        assert (y + h) % bs == 0 or dy + h == height
        src_tiles_y = -(-s["H"] // bs)
        tx, ty = mine // tiles_y, mine % tiles_y
        src = (tx - dx // bs + x // bs) * src_tiles_y + (ty - dy // bs + y // bs)
        counts[mine] = c[src]
        rec[mine] = r[src]
    codes = []
    for ch in range(3):
        for step in range(k):
            live = counts[:, ch] > step
            for half in (0, 1):
                codes.append(rec[live, ch, step, half])
    return ia.write_compressed(width, height, k, bs, head["quant"].astype(np.float64), counts.astype(np.uint16).reshape(-1), codes)


def check_coverage(ia):
    """what the lists are there for"""
    t0, t1, _ = region_cases.tile_range((224, 64, 37, 24), H)
    assert t0 < 1024 < t1
    main = container()
    for name, (blobs, parts, width, height) in lists().items():
        if name.startswith("edit") or name.startswith("move") or name == "overlap":
            assert expected(name) != main, name
    blobs, parts, width, height = lists()["overlap"]
    owner = owners(blobs, parts, width, height)
    assert [p for p in range(len(parts)) if not (owner == p).any()] == [0]
    assert ia.container_info(other_quality_container())[2:] == (K, 8)
    assert not np.array_equal(ia.read_compressed(other_quality_container())["quant"], ia.read_compressed(main)["quant"])
