"""Transcode on the host (no GPU): mpc_transcode_container -- which defines what mpc_transcode_views_indexed computes on the device --
against the oracle's encode of the cropped pixels, against the numpy model of transcode_cases, and against its own identities.  Every
equality is exact: the result is not close to a fresh encode, it is the fresh encode's bytes."""
import numpy as np
import pytest

import parse_cases
import region_cases
import transcode_cases as tc
import view_cases
from container_cases import corpus as _corpus


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def main(oracle):
    return region_cases.container()


@pytest.fixture(scope="module")
def real(oracle):
    return parse_cases.real(oracle)


def test_transcode_is_the_encode_of_the_crop(ia, oracle, main):
    sizes = {}
    for rect in tc.RECTS:
        for m in tc.STEPS:
            got = ia.transcode_container(main, (rect, m, 0))
            assert got == tc.fresh(rect, m), (rect, m)
            assert ia.container_info(got) == (rect[2], rect[3], tc.K, 8), (rect, m)
            sizes[rect, m] = len(got)
    assert ia.transcode_container(main, (tc.RECTS[0], 0, 0)) == main
    # the sizes measured when the identity was first checked with the numpy model
    assert [sizes[r, 0] for r in tc.RECTS] == [26930, 834, 3731, 217, 782, 212, 268]


def test_transcode_is_the_model(ia, real, main):
    for rect in tc.RECTS + (tc.WHOLE,):
        for m in tc.STEPS:
            assert ia.transcode_container(main, (rect, m, 0)) == tc.model(main, (rect, m, 0)), (rect, m)
    inputs = list(parse_cases.synthetic().items()) + real + [("golden", parse_cases.golden_mn())]
    for name, blob in inputs:
        w, h, k, bs = ia.container_info(blob)
        assert bs == 8
        tx, ty = -(-w // 8), -(-h // 8)
        # one interior rectangle where the frame has an interior, and the ragged (or last) corner tile
        inner = (8 * (tx // 4), 8 * (ty // 4), 8 * max(tx // 2, 1), 8 * max(ty // 2, 1)) if tx >= 4 and ty >= 4 else tc.WHOLE
        corner = (8 * (tx - 1), 8 * (ty - 1), w - 8 * (tx - 1), h - 8 * (ty - 1))
        for view in ((tc.WHOLE, 0, 0), (inner, 0, 0), (inner, 1, 0), (corner, max(k // 2, 1), 0)):
            assert ia.transcode_container(blob, view) == tc.model(blob, view), (name, view)


def test_whole_frame_identities(ia, real, main):
    for name, blob in [("main", main), ("small", view_cases.small())] + real:
        k = ia.container_info(blob)[2]
        w, h = ia.container_info(blob)[:2]
        again = ia.truncate_container(blob, k)                      # what coding the parsed container again gives
        assert again == blob, name                                  # an encoder's container: the input itself
        for rect in (tc.WHOLE, (0, 0, w, h)):
            assert ia.transcode_container(blob, (rect, 0, 0)) == again, name
            assert ia.transcode_container(blob, (rect, k + 3, 0)) == again, name
            for m in sorted({1, max(k // 2, 1), k}):
                assert ia.transcode_container(blob, (rect, m, 0)) == ia.truncate_container(blob, m), (name, m)
    # a container no encoder wrote (random symbols): still what coding the parse again gives
    for name, blob in parse_cases.synthetic().items():
        k = ia.container_info(blob)[2]
        assert ia.transcode_container(blob, (tc.WHOLE, 0, 0)) == ia.truncate_container(blob, k), name
        assert ia.transcode_container(blob, (tc.WHOLE, 1, 0)) == ia.truncate_container(blob, 1), name


def test_transcodes_compose(ia, main):
    outer = tc.INTERIOR                                             # (40, 64, 168, 96)
    mid = ia.transcode_container(main, (outer, 0, 0))
    for inner in ((0, 0, 168, 96), (8, 16, 64, 40), (160, 88, 8, 8), (56, 0, 80, 96)):
        direct = (outer[0] + inner[0], outer[1] + inner[1], inner[2], inner[3])
        for m in (0, 1, 3):
            want = ia.transcode_container(main, (direct, m, 0))
            assert ia.transcode_container(mid, (inner, m, 0)) == want, (inner, m)
            # cutting steps commutes with cropping
            assert ia.transcode_container(ia.transcode_container(main, (outer, m, 0)), (inner, 0, 0)) == want, (inner, m)
            assert ia.transcode_container(ia.transcode_container(main, (tc.WHOLE, m, 0)), (direct, 0, 0)) == want, (inner, m)
            if m:
                assert ia.truncate_container(ia.transcode_container(main, (direct, 0, 0)), m) == want, (inner, m)
    # a ragged edge stays legal through the composition where it is the frame's own
    corner = ia.transcode_container(main, ((224, 64, 37, 213), 0, 0))
    assert ia.transcode_container(corner, ((32, 208, 5, 5), 2, 0)) == ia.transcode_container(main, ((256, 272, 5, 5), 2, 0))


def test_block_size_four(ia, oracle):
    pixels, blob = tc.bs4()
    w, h, k, bs, quality = tc.BS4
    assert ia.container_info(blob) == (w, h, k, bs)
    x, y, rw, rh = tc.BS4_RECT
    octx = oracle.OracleContext(k, bs, quality)
    for rect in (tc.BS4_RECT, (0, 0, w, h), (28, 20, 2, 2), (4, 8, 8, 4)):
        cropped = bytes(octx.encode_image(np.ascontiguousarray(pixels[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]])))
        for m in (0, 1, 3):
            want = cropped if m == 0 else view_cases.truncated(cropped, m)
            got = ia.transcode_container(blob, (rect, m, 0))
            assert got == want and got == tc.model(blob, (rect, m, 0)), (rect, m)
    for rect in ((8, 4, 22, 13), (2, 4, 4, 4), (8, 8, 8, 8)):           # aligned to 8 is aligned to 4; the others are not
        if tc.aligned(rect, w, h, bs):
            ia.transcode_container(blob, (rect, 0, 0))
        else:
            with pytest.raises(ia.MpcError) as e:
                ia.transcode_container(blob, (rect, 0, 0))
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT, rect


def test_argument_errors(ia, main):
    for view in tc.ARGUMENT_ERRORS:
        with pytest.raises(ia.MpcError) as e:
            ia.transcode_container(main, view)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, view
    for rect in tc.RECTS:                                           # and the list above is not refused for another reason
        assert tc.aligned(rect, tc.W, tc.H, 8)
    for (rect, m, s) in tc.ARGUMENT_ERRORS:
        assert m < 0 or s != 0 or not tc.aligned(rect, tc.W, tc.H, 8) or rect == tc.WHOLE, (rect, m, s)


def test_a_length_above_k_is_refused(ia, main):
    s = ia.read_compressed(main)
    lengths = s["lengths"].copy()
    at = int(np.flatnonzero(lengths == tc.K)[0])
    lengths[at] = tc.K + 1                                          # the streams stay what the lengths, cut to K, promise
    bad = ia.write_compressed(s["W"], s["H"], s["K"], s["bs"], s["quant"].astype(np.float64), lengths, s["codes"])
    ia.read_compressed(bad)
    for rect in (tc.WHOLE, (0, 0, 8, 8)):                           # anywhere in the frame, not only in the rectangle
        with pytest.raises(ia.MpcError) as e:
            ia.transcode_container(bad, (rect, 1, 0))
        assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid bitstream"), rect


def test_damaged_containers_get_read_compressed_verdict(ia, oracle):
    for n, blob, xs in _corpus(oracle):
        refused = accepted = 0
        for k, x in enumerate(xs):
            try:
                s = ia.read_compressed(x)
            except ia.MpcError:
                for view in ((tc.WHOLE, 0, 0), (tc.WHOLE, 1, 0)):
                    with pytest.raises(ia.MpcError) as e:
                        ia.transcode_container(x, view)
                    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid input data"), (n, k)
                refused += 1
                continue
            if s["lengths"].max(initial=0) > s["K"]:                # parses, and no decoder takes it: the transcode's own refusal
                with pytest.raises(ia.MpcError) as e:
                    ia.transcode_container(x, (tc.WHOLE, 0, 0))
                assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid bitstream"), (n, k)
                continue
            for view in ((tc.WHOLE, 0, 0), (tc.WHOLE, 1, 0)):
                assert ia.transcode_container(x, view) == tc.model(x, view), (n, k, view)
            accepted += 1
        assert refused > 10 and accepted >= 1, n
