"""The frame layouts of tests/layout_cases.py, checked on the CPU: every case really reaches the branch of the refill its row
names, `embed` puts every pixel where the layout says and poison everywhere else, and the two poisons differ in every byte a
correct encoder never reads.  test_gpu_frame_layouts.py relies on all of it: a case that silently lost its property (a stride that
became a multiple of 8, a width that became whole) would still pass there and test nothing."""
import numpy as np
import pytest

import layout_cases as lc

IDS = [c.name for c in lc.CASES]


def _frames(case):
    """content without the oracle: every byte distinct from its neighbours often enough, seeded by the case"""
    L = case.layout
    return np.random.default_rng(case.seed).integers(0, 256, (L.frames, L.H, L.W, 3)).astype(np.uint8)


def test_the_issue_table_is_all_there():
    want = {"pad8": (64, 48, 200, 0), "pad8-ragged-x": (44, 400, 136, 0), "pad8-ragged-xy": (70, 50, 216, 0), "pad-odd": (64, 48, 197, 0),
            "offset-odd-1": (64, 48, 192, 1), "offset-odd-3": (64, 48, 192, 3), "offset-odd-4": (64, 48, 192, 4),
            "narrow-3x5": (3, 5, 64, 0), "narrow-8x8": (8, 8, 64, 0), "K32": (44, 400, 136, 0)}
    for name, (W, H, rs, off) in want.items():
        L = lc.BY_NAME[name].layout
        assert (L.W, L.H, L.row_stride, L.offset, L.frames) == (W, H, rs, off, 1), name
    batches = {"batch-pad": (4, 70, 50, 216, 216 * 50 + 40), "batch-odd": (3, 64, 48, 192, 3 * 64 * 48 + 3),
               "batch-ragged": (4, 139, 100, 417, 41700)}
    for name, (n, W, H, rs, fs) in batches.items():
        L = lc.BY_NAME[name].layout
        assert (L.frames, L.W, L.H, L.row_stride, L.frame_stride, L.offset) == (n, W, H, rs, fs, 0), name
    crops = [c for c in lc.CASES if c.name.startswith("crop-")]
    assert sorted((c.layout.W, c.layout.H) + c.claims["window"] for c in crops) == sorted(
        [(40, 24, 8, 8), (40, 24, 5, 3), (40, 24, 56, 40), (41, 27, 8, 8), (41, 27, 5, 3), (41, 27, 55, 37)])
    assert all(c.layout.row_stride == 288 for c in crops)
    assert lc.BY_NAME["K32"].K == 32 and all(c.K == 8 for c in lc.CASES if c.name != "K32")
    assert len(set(IDS)) == len(IDS)
    assert set(lc.STEPS_PATH_CASES) <= set(IDS)


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_case_has_the_property_it_claims(case):
    L, claims = case.layout, case.claims
    tiles_x, tiles_y = lc.tiles_of(L)
    q = lc.queue_whole(L)
    assert L.row_stride >= 3 * L.W
    assert L.frames == 1 or L.frame_stride >= L.row_stride * L.H
    # the flag, and exactly why it is clear
    assert lc.flag_set(L) == claims["flag"]
    assert lc.flag_reasons(L) == set(claims["clear_by"])
    if claims.get("all_whole"):
        assert q.all()
    if claims.get("edge_tiles"):
        assert claims["flag"] and (~q).any() and q.any()           # both fetches in one launch
    if "whole_run" in claims:
        assert lc.longest_run(q) >= claims["whole_run"]
    if claims.get("ragged_x"):
        assert L.W % 8 != 0
    if claims.get("ragged_y"):
        assert L.H % 8 != 0
    if "tile0_whole" in claims:
        assert lc.whole(0, 0, L.W, L.H) == claims["tile0_whole"]
    if "frame_gap" in claims:
        assert L.frame_stride - L.row_stride * L.H == claims["frame_gap"]
    if claims.get("tight"):
        assert L.row_stride == 3 * L.W and L.frame_stride == 3 * L.W * L.H
    if "window" in claims:
        x0, y0 = claims["window"]
        assert L.offset == y0 * 3 * lc.PARENT_W + 3 * x0 and L.row_stride == 3 * lc.PARENT_W
        assert 0 <= x0 and x0 + L.W <= lc.PARENT_W and 0 <= y0 and y0 + L.H <= lc.PARENT_H
    for (a, b) in case.stripes:
        assert 0 < a < b <= tiles_y


def test_pad8_ragged_x_mixes_the_two_fetches():
    """a wave takes up to 16 consecutive queue entries per group: 250 whole tiles in a row fill whole waves that take the 8-byte
    path, and the sixth column's 50 edge tiles take the byte path under the same flag"""
    L = lc.BY_NAME["pad8-ragged-x"].layout
    q = lc.queue_whole(L)
    assert lc.flag_set(L) and lc.tiles_of(L) == (6, 50)
    assert lc.longest_run(q) == 250 and int((~q).sum()) == 50
    assert q[:250].all() and not q[250:].any()
    for (a, b) in lc.BY_NAME["pad8-ragged-x"].stripes:
        qs = lc.queue_whole(L, a, b)
        assert lc.longest_run(qs) >= 32 and (~qs).any()


def test_short_columns_mix_whole_and_edge_tiles_inside_a_refill():
    """pad8-ragged-xy and batch-pad: columns of 7 tiles whose last is an edge tile, so no 16 consecutive queue entries are all
    whole -- every full refill of a wave ballots a tile that is not"""
    for name in ("pad8-ragged-xy", "batch-pad"):
        L = lc.BY_NAME[name].layout
        q = lc.queue_whole(L)
        assert lc.flag_set(L) and lc.longest_run(q) < 16 and q.any()
    L = lc.BY_NAME["batch-pad"].layout
    ends_ragged = [s for s in lc.BY_NAME["batch-pad"].stripes if s[1] == lc.tiles_of(L)[1]]
    assert ends_ragged and L.H % 8 != 0
    assert not lc.queue_whole(L, *ends_ragged[0]).all()


def test_flag_is_clear_for_exactly_the_reason_named():
    for name, why in (("offset-odd-1", "pointer"), ("offset-odd-3", "pointer"), ("offset-odd-4", "pointer"), ("pad-odd", "row_stride"),
                      ("batch-odd", "frame_stride")):
        L = lc.BY_NAME[name].layout
        assert lc.flag_reasons(L) == {why}, name
        # ... and the same layout with that one thing put right has the flag set
        fixed = {"pointer": L._replace(offset=0), "row_stride": L._replace(row_stride=(L.row_stride + 7) // 8 * 8),
                 "frame_stride": L._replace(frame_stride=(L.frame_stride + 7) // 8 * 8)}[why]
        assert lc.flag_set(fixed), name
    odd = lc.BY_NAME["batch-odd"].layout
    assert lc.flag_set(odd._replace(frames=1))               # frame_stride counts for batches only
    assert {lc.BY_NAME[f"offset-odd-{o}"].layout.offset % 8 for o in (1, 3, 4)} == {1, 3, 4}
    crops = [c for c in lc.CASES if c.name.startswith("crop-")]
    assert {c.claims["flag"] for c in crops} == {True, False}


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_embed_places_pixels_and_poison(case):
    L = case.layout
    frames = _frames(case)
    zero, start = lc.embed(frames, L, "zero")
    rand, start2 = lc.embed(frames, L, "random")
    assert start == start2 == lc.margin(L) + L.offset and lc.margin(L) % 8 == 0
    assert zero.shape == rand.shape and zero.dtype == rand.dtype == np.uint8
    # slicing the view back out returns the tight frames
    for parent in (zero, rand):
        assert (lc.extract(parent, start, L) == frames).all()
        for f in range(L.frames):
            v = lc.host_view(parent, start, L, f)
            assert v.strides == (L.row_stride, 3, 1) and (v == frames[f]).all()
            assert (np.ascontiguousarray(v) == frames[f]).all()
    # larger than the view on every side by at least one row stride and 64 bytes
    assert start - L.offset >= L.row_stride + 64
    assert zero.size - (start + lc.span(L)) >= L.row_stride + 64
    # the poisons: all zero; never zero, never the neighbouring pixel; different in every non-pixel byte
    is_pixel = np.zeros(zero.size, bool)
    is_pixel[(start + lc.pixel_index(L)).reshape(-1)] = True
    assert int(is_pixel.sum()) == frames.size
    assert (zero[~is_pixel] == 0).all()
    assert (rand[~is_pixel] != 0).all()
    assert (zero[~is_pixel] != rand[~is_pixel]).all()
    assert (zero[is_pixel] == rand[is_pixel]).all()
    prev, nxt = lc._neighbours(rand, is_pixel)
    assert ((rand != prev) & (rand != nxt))[~is_pixel].all()
    if L.row_stride > 3 * L.W or (L.frames > 1 and L.frame_stride > L.row_stride * L.H):
        assert (~is_pixel[start:start + lc.span(L)]).any()          # padding inside the view itself


def test_neighbours_on_a_hand_made_buffer():
    buf = np.array([9, 1, 2, 9, 9, 3, 9], np.uint8)
    is_pixel = np.array([0, 1, 1, 0, 0, 1, 0], bool)
    prev, nxt = lc._neighbours(buf, is_pixel)
    assert prev.tolist() == [-1, 1, 2, 2, 2, 3, 3]
    assert nxt.tolist() == [1, 1, 2, 3, 3, 3, -1]


def test_stripe_of_reorders_like_the_encoders():
    frames, tiles_x, tiles_y, a, b = 2, 3, 5, 1, 4
    t = np.arange(frames * tiles_x * tiles_y).reshape(-1, 1) * np.ones((1, 3), np.int64)
    (got,) = lc.stripe_of((t,), frames, tiles_x, tiles_y, a, b)
    want = [f * tiles_x * tiles_y + tx * tiles_y + ty for f in range(frames) for tx in range(tiles_x) for ty in range(a, b)]
    assert got[:, 0].tolist() == want and got.shape == (len(want), 3)
