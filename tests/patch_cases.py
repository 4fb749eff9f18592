"""The model and the cases of the delta stream's tests, shared by the host tests and the device tests (nothing here needs a GPU).

A patch is the ascending list of changed tiles plus the container of their packed frame (include/mpcodec.h, "patch").  Here, in plain
Python and numpy:
  make / parse   the format, version 1, written and read a second time: the library's writer and parser are held to these
  hostile        blobs every parser must refuse, each made from a valid patch by one change
  unpack         the inverse of delta_cases.pack on a frame as it lies in memory (a delta_cases.Layout): listed tile j of the packed
                 frame to tile tiles[j], only the bytes inside the image; `WRONG_UNPACKS` are the mistakes the cases must be able to
                 tell from it (tests/test_patch_cases.py checks that they can)
The shapes, strides, tile sets and frame sequences are delta_cases's."""
import struct

import numpy as np

import delta_cases as dc

HEADER = 40
MAGIC = b"MPCP"
LEADS = (0, 1, 8)                               # the destination's base against an 8-byte boundary
GUARD = 64                                      # bytes in front of the destination that nothing may touch


class Refused(ValueError):
    """what the model's parser raises for a blob the format does not allow"""


def tile_count(w, h):
    return -(-w // 8) * -(-h // 8)


def leb128(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def gaps(tiles):
    """g0 = t0, gj = tj - t(j-1) - 1"""
    tiles = [int(t) for t in tiles]
    return [t - (tiles[j - 1] + 1 if j else 0) for j, t in enumerate(tiles)]


def header(w, h, sequence, key, n, list_bytes, container_bytes, magic=MAGIC, version=1, flags=None, reserved=0):
    return magic + struct.pack("<HHIIIIIIQ", version, (1 if key else 0) if flags is None else flags, w, h, sequence, n, list_bytes, reserved,
                               container_bytes)


def make(w, h, sequence, tiles, container, key=False):
    """the model's writer: tiles ascending (not read for a key patch), container bytes (b"" for an empty patch)"""
    listed = b"" if key else b"".join(leb128(g) for g in gaps(tiles))
    n = tile_count(w, h) if key else len(tiles)
    return header(w, h, sequence, key, n, len(listed), len(container)) + listed + bytes(container)


def container_size(blob):
    """(width, height) of a container's header as the model needs it: the library's own reader of that header"""
    import imageexperiments_amd as ia
    try:
        return ia.container_info(blob)[:2]
    except ia.MpcError:
        raise Refused("the container's header") from None


def parse(blob):
    """the model's parser -> dict(width, height, sequence, key, n, tiles, container_offset, container_bytes, list); Refused otherwise"""
    blob = bytes(blob)
    if len(blob) < HEADER or blob[:4] != MAGIC:
        raise Refused("header")
    version, flags, w, h, sequence, n, list_bytes, reserved, container_bytes = struct.unpack("<HHIIIIIIQ", blob[4:HEADER])
    if version != 1 or flags & ~1 or reserved != 0 or w < 1 or h < 1 or w >= 2**31 or h >= 2**31 or tile_count(w, h) >= 2**31:
        raise Refused("header")
    if len(blob) != HEADER + list_bytes + container_bytes:
        raise Refused("length")
    key, tiles = bool(flags & 1), tile_count(w, h)
    if n > tiles or (key and (n != tiles or list_bytes)) or (not key and n == tiles):
        raise Refused("form")
    if n == 0 and (list_bytes or container_bytes):
        raise Refused("form")
    if n > 0 and container_bytes == 0:
        raise Refused("form")
    listed, at, t = [], HEADER, -1
    if not key:
        for _ in range(n):
            v = 0
            for used in range(6):
                if used == 5 or at == HEADER + list_bytes:
                    raise Refused("varint")
                b = blob[at]
                at += 1
                v |= (b & 0x7F) << (7 * used)
                if not b & 0x80:
                    if used and b == 0:
                        raise Refused("varint")
                    break
            if v >= 2**31:
                raise Refused("varint")
            t += v + 1
            if t >= tiles:
                raise Refused("tile")
            listed.append(t)
        if at != HEADER + list_bytes:
            raise Refused("list")
    if n:
        R, Cc, _, _ = dc.pack_geometry(n)
        if container_size(blob[HEADER + list_bytes:]) != ((w, h) if key else (8 * Cc, 8 * R)):
            raise Refused("container size")
    return dict(width=w, height=h, sequence=sequence, key=int(key), n=n, tiles=tiles, container_offset=HEADER + list_bytes,
                container_bytes=container_bytes, list=list(range(tiles)) if key else listed)


def hostile(valid_tile, valid_key, valid_empty, other_size_container):
    """[(label, blob)]: blobs a parser must refuse, made from three valid patches of one geometry -- a tile patch of at least two
    tiles whose first gap is below 128, a key patch, an empty patch -- and a valid container of a size that is neither the frame's
    nor the tile patch's packed frame's"""
    p = parse(valid_tile)
    w, h, seq, n, tiles = p["width"], p["height"], p["sequence"], p["n"], p["tiles"]
    listed, cont = valid_tile[HEADER:p["container_offset"]], valid_tile[p["container_offset"]:]
    whole = valid_key[HEADER:]

    def tile(n=n, listed=listed, cont=cont, list_bytes=None, container_bytes=None, **kw):
        return header(w, h, seq, False, n, len(listed) if list_bytes is None else list_bytes,
                      len(cont) if container_bytes is None else container_bytes, **kw) + listed + cont

    first = p["list"][0]
    rest = listed[len(leb128(first)):]
    past = p["list"][:-1] + [tiles]                                                # the last tile = tiles
    out = [(f"prefix {k}", valid_tile[:k]) for k in range(len(valid_tile))]
    out += [(f"key prefix {k}", valid_key[:k]) for k in list(range(0, HEADER + 1)) + [len(valid_key) - 1]]
    out += [(f"empty prefix {k}", valid_empty[:k]) for k in range(HEADER)]
    out += [("wrong magic", tile(magic=b"MPCQ")), ("wrong version", tile(version=2)), ("version 0", tile(version=0)),
            ("a reserved flag bit", tile(flags=2)), ("a reserved flag bit beside key", header(w, h, seq, True, tiles, 0, len(whole), flags=0x8001) + whole),
            ("a nonzero reserved word", tile(reserved=1)),
            ("list_bytes one too small", tile(list_bytes=len(listed) - 1)), ("list_bytes one too large", tile(list_bytes=len(listed) + 1)),
            ("list_bytes one too small, the length kept", tile(list_bytes=len(listed) - 1, container_bytes=len(cont) + 1)),
            ("list_bytes one too large, the length kept", tile(list_bytes=len(listed) + 1, container_bytes=len(cont) - 1)),
            ("a 6-byte varint", tile(listed=bytes([first | 0x80, 0x80, 0x80, 0x80, 0x80, 0x00]) + rest)),
            ("a trailing 0x00 group", tile(listed=bytes([first | 0x80, 0x00]) + rest)),
            ("a value of 2^31", tile(listed=bytes([0x80, 0x80, 0x80, 0x80, 0x08]) + rest)),
            ("a value of 2^35 - 1", tile(listed=bytes([0xFF, 0xFF, 0xFF, 0xFF, 0x7F]) + rest)),
            ("last tile = tiles", tile(listed=b"".join(leb128(g) for g in gaps(past)))),
            ("n one too small", tile(n=n - 1)), ("n one too large", tile(n=n + 1)),
            ("a key patch with a list", header(w, h, seq, True, tiles, len(listed), len(whole)) + listed + whole),
            ("a key patch with n one short", header(w, h, seq, True, tiles - 1, 0, len(whole)) + whole),
            ("an empty patch with a container", header(w, h, seq, False, 0, 0, len(cont)) + cont),
            ("an empty patch with a list", header(w, h, seq, False, 0, 1, 0) + b"\0"),
            ("a tile patch without a container", tile(cont=b"")),
            ("n == tiles without the key flag", header(w, h, seq, False, tiles, 0, len(whole)) + whole),
            ("n == tiles without the key flag, listed",
             header(w, h, seq, False, tiles, tiles, len(whole)) + bytes(tiles) + whole),
            ("trailing bytes", valid_tile + b"\0"), ("trailing bytes behind an empty patch", valid_empty + b"\0"),
            ("container_bytes beyond the blob", tile(container_bytes=len(cont) + 1)),
            ("container_bytes far beyond the blob", tile(container_bytes=2**63)),
            ("container_bytes that wraps", tile(container_bytes=2**64 - HEADER - len(listed))),
            ("width 0", header(0, h, seq, False, 0, 0, 0)), ("height 0", header(w, 0, seq, False, 0, 0, 0)),
            ("2^31 tiles and more", header(2**31 - 1, 2**31 - 1, seq, False, 0, 0, 0)),
            ("a container that is none", tile(cont=b"\xff" * len(cont))),
            ("a tile patch's container of another size", tile(cont=other_size_container)),
            ("a key patch's container of another size", header(w, h, seq, True, tiles, 0, len(other_size_container)) + other_size_container)]
    return out


# ---- unpack: the model on memory ----
WRONG_UNPACKS = ("writes a ragged tile's black fill past the image", "writes padding tiles", "row-major packed order", "overwrites stride padding",
                 "drops the partial chunk at the right edge")


def unpack_raw(packed, tiles, raw, off, stride, w, h, rows=dc.PACK_ROWS, mistake=None):
    """the model: a copy of the memory `raw` (uint8, 1-D; pixel (x, y) of the w x h frame at off + y * stride + 3 * x) with listed tile j
    of the packed frame [8R, 8C, 3] written to tile tiles[j]; an entry outside the frame's tiles writes nothing -> (memory, an entry was
    outside the frame)"""
    out = np.array(raw)
    tx, ty = dc.grid(w, h)
    R, Cc, _, _ = dc.pack_geometry(len(tiles), rows)
    rows_of = np.asarray(packed, np.uint8).reshape(8 * R, 24 * Cc)
    bad = False
    jobs = list(enumerate(tiles))
    if mistake == "writes padding tiles":                                          # a missing entry read as tile 0, as a zeroed list gives it
        jobs += [(j, 0) for j in range(len(tiles), R * Cc)]
    for j, t in jobs:
        if not 0 <= t < tx * ty:
            bad = True
            continue
        px, py = (j % Cc, j // Cc) if mistake == "row-major packed order" else (j // R, j % R)
        cx, cy = divmod(int(t), ty)
        for r in range(8):
            y = cy * 8 + r
            nb = min(max(3 * w - 24 * cx, 0), 24)
            if mistake == "writes a ragged tile's black fill past the image":
                nb = 24
            elif y >= h:
                continue
            elif mistake == "overwrites stride padding":
                nb = min(max(max(stride, 3 * w) - 24 * cx, 0), 24)
            elif mistake == "drops the partial chunk at the right edge":
                nb = nb // 8 * 8
            at = off + y * stride + 24 * cx
            nb = min(nb, out.size - at)                                            # a wrong variant stays inside the memory it is given
            if nb > 0:
                out[at:at + nb] = rows_of[py * 8 + r, 24 * px:24 * px + nb]
    return out, bad


def unpack(packed, tiles, frame, rows=dc.PACK_ROWS):
    """the inverse of delta_cases.pack on pixel arrays: a copy of the h x w x 3 `frame` with the listed tiles taken from the packed frame"""
    h, w = frame.shape[:2]
    out, _ = unpack_raw(packed, tiles, np.ascontiguousarray(frame).reshape(-1), 0, 3 * w, w, h, rows)
    return out.reshape(h, w, 3)


def tile_lists(name):
    """{label: tiles}: delta_cases's tile sets without the empty one (first, last and all among them)"""
    return {label: tiles for label, tiles in dc.tile_sets(name).items() if tiles}


def unpack_cases(name):
    """[(label, old Layout, new pixels, tiles, rows)]: every stride kind x every base offset x every tile list.  The destination holds
    another frame's pixels, GUARD bytes and more in front, stride gaps and the room behind full of random bytes"""
    w, h, _ = dc.SHAPES[name]
    old, new = dc.frame(w, h, 11), dc.frame(w, h, 12)
    out = []
    for s, kind in enumerate(dc.STRIDES):
        for lead in LEADS:
            for label, tiles in tile_lists(name).items():
                out.append((f"{kind} +{lead} {label}", dc.Layout(old, kind, GUARD + lead, 500 + s), new, tiles, dc.PACK_ROWS))
        out.append((f"{kind} rows 3", dc.Layout(old, kind, GUARD, 600 + s), new, tile_lists(name)["random"], 3))
    return out


def stream(name, encode_image):
    """[(frame, list or None for a key patch, patch)] for delta_cases.sequence(name): the patches a sender that sees only these frames
    must emit, sequence 0, 1, ...; encode_image(pixels) -> container"""
    frames, out = dc.sequence(name), []
    w, h, _ = dc.SHAPES[name]
    for i, px in enumerate(frames):
        listed = None if i == 0 else [int(t) for t in dc.changed_tiles(frames[i - 1], px)]
        if listed is None or len(listed) == tile_count(w, h):
            out.append((px, None, make(w, h, i, None, encode_image(px), key=True)))
        elif not listed:
            out.append((px, listed, make(w, h, i, [], b"")))
        else:
            out.append((px, listed, make(w, h, i, listed, encode_image(dc.pack(px, listed)))))
    return out
