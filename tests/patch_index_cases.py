"""The model and the cases of the tests of patch format version 2, shared by the host tests and the device tests (nothing here needs a
GPU).

A version-2 patch is a version-1 patch (tests/patch_cases.py) with version = 2, the reserved word at 28 holding index_bytes (> 0) and
that many bytes behind the container: the container's seek index, which a receiver hands to the decoder so that the entropy codes are
parsed on the device (include/mpcodec.h, "patch index").  Here, in plain Python:
  make / parse       the format written and read a second time; version 1 goes through patch_cases unchanged
  strip / add_index  the host definition of what a sender that attaches the index does
  hostile            version-2 blobs every parser must refuse, each made from a valid one by a single change
  damaged            index sections that are wrong in ways a decoder must survive: the index is a hint
  stream             patch_cases.stream and behind it frames whose lists are long: 424 of 425 tiles (seven packed columns; the key patch
                     of that shape has a lengths stream of 1275 symbols, 40 chunks of 32 with the last one short), 65 tiles (a second
                     packed column), a third of the tiles
The shapes are delta_cases's."""
import struct

import numpy as np

import delta_cases as dc
import patch_cases as pc

HEADER = pc.HEADER
INTERVALS = (32, 0)                             # the smallest interval, and the library's default


def fields(blob):
    """(version, flags, w, h, sequence, n, list_bytes, word 28, container_bytes) of a header"""
    return struct.unpack("<HHIIIIIIQ", bytes(blob[4:HEADER]))


def with_fields(blob, version=None, word28=None):
    """the blob with its version word and / or the word at 28 rewritten"""
    out = bytearray(blob)
    if version is not None:
        out[4:6] = struct.pack("<H", version)
    if word28 is not None:
        out[28:32] = struct.pack("<I", word28)
    return bytes(out)


def make(w, h, sequence, tiles, container, key=False, index=None):
    """the model's writer: patch_cases.make, and with an index (bytes, not empty) version 2 with that section appended"""
    v1 = pc.make(w, h, sequence, tiles, container, key)
    if not index:
        return v1
    return with_fields(v1, version=2, word28=len(index)) + bytes(index)


def parse(blob):
    """the model's parser -> patch_cases.parse's dict of the stripped patch plus version, index_offset, index_bytes; pc.Refused otherwise"""
    blob = bytes(blob)
    if len(blob) < HEADER or blob[:4] != pc.MAGIC:
        raise pc.Refused("header")
    version, word28 = fields(blob)[0], fields(blob)[7]
    if version == 1:
        return dict(pc.parse(blob), version=1, index_offset=0, index_bytes=0)
    if version != 2 or word28 == 0 or word28 > len(blob) - HEADER:
        raise pc.Refused("header")
    body = len(blob) - word28
    p = pc.parse(with_fields(blob[:body], version=1, word28=0))      # the length, the forms, the list, the container's header
    if p["n"] == 0:
        raise pc.Refused("a version-2 empty patch")
    return dict(p, version=2, index_offset=body, index_bytes=word28)


def strip(blob):
    """the version-1 patch of a valid patch"""
    parse(blob)
    return cut(blob)


def cut(blob):
    """strip by the header's words alone, for a patch that need not be valid: what it says its index section is goes, the rest stays"""
    blob = bytes(blob)
    version, word28 = fields(blob)[0], fields(blob)[7]
    return blob if version != 2 else with_fields(blob[:len(blob) - word28], version=1, word28=0)


def add_index(blob, interval=0, index_min_bytes=0):
    """the model of mpc_patch_add_index: the stripped patch, and behind it the library's container_index of its container where the
    container has at least max(index_min_bytes, 1) bytes and the index does not say "serial only" """
    import imageexperiments_amd as ia
    v1 = strip(blob)
    p = pc.parse(v1)
    if p["container_bytes"] < max(index_min_bytes, 1):
        return v1
    try:
        index = ia.container_index(v1[p["container_offset"]:], interval)
    except ia.MpcError:
        return v1                                                    # a container that does not parse has no index
    if ia.index_info(index)["serial_only"]:
        return v1
    return with_fields(v1, version=2, word28=len(index)) + index


def hostile(valid_tile, valid_key, valid_empty):
    """[(label, blob)]: blobs a parser must refuse, each a single change of a valid version-2 tile patch, a valid version-2 key patch or a
    valid (version-1) empty patch"""
    pt, pk = parse(valid_tile), parse(valid_key)
    assert pt["version"] == pk["version"] == 2 and not pt["key"] and pk["key"] and parse(valid_empty)["n"] == 0
    index = valid_tile[pt["index_offset"]:]
    out = [(f"prefix {k}", valid_tile[:k]) for k in range(len(valid_tile))]
    out += [(f"key prefix {k}", valid_key[:k]) for k in list(range(HEADER + 1)) + [pk["index_offset"], len(valid_key) - 1]]
    for label, good, p in (("tile", valid_tile, pt), ("key", valid_key, pk)):
        out += [(f"{label}: index_bytes 0", with_fields(good, word28=0)),
                (f"{label}: index_bytes 0 and the section gone", with_fields(good[:p["index_offset"]], word28=0)),
                (f"{label}: one byte short", good[:-1]), (f"{label}: one byte long", good + b"\0"),
                (f"{label}: index_bytes one too small", with_fields(good, word28=p["index_bytes"] - 1)),
                (f"{label}: index_bytes one too large", with_fields(good, word28=p["index_bytes"] + 1)),
                (f"{label}: index_bytes the whole body", with_fields(good, word28=len(good) - HEADER)),
                (f"{label}: index_bytes 2^32 - 1", with_fields(good, word28=2**32 - 1)),
                (f"{label}: version 1 with index_bytes set", with_fields(good, version=1)),
                (f"{label}: version 3", with_fields(good, version=3)), (f"{label}: version 0x0102", with_fields(good, version=0x0102)),
                (f"{label}: the index section in front of the container",
                 good[:p["container_offset"]] + good[p["index_offset"]:] + good[p["container_offset"]:p["index_offset"]])]
    w, h, seq = pt["width"], pt["height"], pt["sequence"]
    out += [("version 2 with n = 0", with_fields(valid_empty, version=2)),
            ("version 2 with an index on an empty form", with_fields(valid_empty, version=2, word28=len(index)) + index),
            ("version 2 with n = 0 and the tile patch's container",
             pc.header(w, h, seq, False, 0, 0, pt["container_bytes"], version=2, reserved=len(index)) + valid_tile[pt["container_offset"]:]),
            ("version 1 empty with index_bytes set", with_fields(valid_empty, word28=len(index)) + index)]
    return out


def damaged(patch, other_index, seed=0):
    """[(label, patch, the route must be 1)]: the version-2 patch with its index section replaced by something that is not this
    container's index; every one of them is a valid patch"""
    p = parse(patch)
    assert p["version"] == 2
    head, index = bytes(patch)[:p["index_offset"]], bytearray(patch[p["index_offset"]:])

    def put(section):
        return with_fields(head, word28=len(section)) + bytes(section)

    magic = bytearray(index)
    magic[0] ^= 1
    out = [("the magic flipped", put(magic), True)]
    n_streams = struct.unpack("<I", index[40:44])[0]
    first = 56 + 64 * n_streams                                       # the first checkpoint: of the lengths stream, which every container has
    assert len(index) >= first + 8
    moved = bytearray(index)
    moved[first] ^= 1
    out.append(("a checkpoint off by one bit", put(moved), False))
    out.append(("another patch's index", put(other_index), False))
    out.append(("cut to its header", put(index[:56]), False))
    out.append(("random bytes", put(np.random.default_rng(seed).integers(0, 256, len(index), dtype=np.uint8).tobytes()), False))
    return out


def frames(name):
    """delta_cases.sequence(name) and behind it frames whose lists are long, then one equal to its predecessor"""
    out = list(dc.sequence(name))
    sets = dc.tile_sets(name)
    for s, label in enumerate(("all but one", "65", "random", "checkerboard")):
        if label in sets and 1 < len(sets[label]) < pc.tile_count(*dc.SHAPES[name][:2]):
            out.append(dc.change_tiles(out[-1], sets[label], 40 + s))
    out.append(np.array(out[-1]))
    return out


def stream(name, encode_image):
    """[(frame, list or None for a key patch, version-1 patch)] for frames(name), as patch_cases.stream makes them for its frames (whose
    stream this one begins with)"""
    w, h, _ = dc.SHAPES[name]
    out = pc.stream(name, encode_image)
    seq = frames(name)
    for i in range(len(out), len(seq)):
        listed = [int(t) for t in dc.changed_tiles(seq[i - 1], seq[i])]
        assert len(listed) < pc.tile_count(w, h)
        out.append((seq[i], listed, pc.make(w, h, i, listed, encode_image(dc.pack(seq[i], listed)) if listed else b"")))
    return out
