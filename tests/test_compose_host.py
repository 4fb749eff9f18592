"""mpc_compose_container, the host definition of a compose: against the numpy model and the oracle's encode of the pasted pixels, the
identities, block size 4, damaged sources and every refusal with its text.  Nothing here needs a GPU."""
import numpy as np
import pytest

import compose_cases as cc
import transcode_cases as tc


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def test_the_cases_cover_what_they_are_for(ia, oracle):
    cc.check_coverage(ia)


@pytest.mark.parametrize("name", cc.NAMES)
def test_compose_is_the_model_and_the_encode_of_the_pasted_pixels(ia, oracle, name):
    blobs, parts, width, height = cc.lists()[name]
    got = ia.compose_container(blobs, parts, width, height)
    assert got == cc.model(blobs, parts, width, height)
    assert got == cc.expected(name)
    assert ia.container_info(got) == (width, height, cc.K, 8)


def test_identities(ia, oracle):
    main = cc.container()
    assert ia.compose_container([main], [(0, None, 0, 0)], cc.W, cc.H) == main
    blobs, parts, width, height = cc.lists()["quadrants"]
    assert ia.compose_container(blobs, parts, width, height) == main
    assert len(ia.compose_container(*cc.lists()["side by side"])) == len(cc.expected("side by side"))
    # compose and transcode commute: a rectangle of a composition is the composition of the rectangles
    rect = (40, 64, 168, 96)
    blobs, parts, width, height = cc.lists()["edit %s" % ((176, 40, 40, 160),)]
    whole = ia.transcode_container(ia.compose_container(blobs, parts, width, height), (rect, 0, 0))
    # the edit (176, 40, 40, 160) meets the rectangle in (176, 64, 32, 96), which lands at (136, 0) of it
    pieces = [ia.transcode_container(blobs[0], (rect, 0, 0)), ia.transcode_container(blobs[1], ((176, 64, 32, 96), 0, 0))]
    assert ia.compose_container(pieces, [(0, None, 0, 0), (1, None, 136, 0)], rect[2], rect[3]) == whole


def test_block_size_4(ia, oracle):
    pixels, blob = tc.bs4()
    w, h, k, bs, quality = tc.BS4
    assert ia.compose_container([blob], [(0, None, 0, 0)], w, h) == blob
    # the rectangle (8, 4, 22, 12) moved up to (8, 0): its ragged right edge stays on the frame's
    parts = [(0, None, 0, 0), (0, tc.BS4_RECT, 8, 0)]
    got = ia.compose_container([blob], parts, w, h)
    assert got == cc.model([blob], parts, w, h)
    assert got == bytes(oracle.OracleContext(k, bs, quality).encode_image(cc.pasted([pixels], parts, w, h)))
    assert got != blob
    with pytest.raises(ia.MpcError, match="part 1: .*not aligned"):
        ia.compose_container([blob], [(0, None, 0, 0), (0, (0, 0, 4, 4), 8, 2)], w, h)


def test_a_part_that_owns_nothing_is_not_read(ia, oracle):
    blobs, parts, width, height = cc.lists()["overlap"]
    want = cc.expected("overlap")
    other = blobs[1]
    # part 0 owns no tile; give it a source of its own whose body is cut in half
    damaged = other[:len(other) // 2]
    assert ia.container_info(damaged) == ia.container_info(other)
    with pytest.raises(ia.MpcError):
        ia.read_compressed(damaged)
    trio = (blobs[0], other, damaged)
    assert ia.compose_container(trio, [(2,) + parts[0][1:]] + list(parts[1:]), width, height) == want
    # the same damage where a part owns tiles: the lowest owning part that names it
    with pytest.raises(ia.MpcError, match=": part 2: Invalid input data$") as e:
        ia.compose_container((blobs[0], damaged), parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM
    with pytest.raises(ia.MpcError, match=": part 1: Invalid input data$"):
        ia.compose_container((blobs[0][:len(blobs[0]) // 2], other), parts, width, height)
    # a header that does not parse is refused whether or not a part names the source
    with pytest.raises(ia.MpcError, match=": source 2: Invalid input data$") as e:
        ia.compose_container((blobs[0], other, b"\0" * 40), parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM


def test_a_length_above_K(ia, oracle):
    bad = cc.length_above_K()
    ia.read_compressed(bad)                                         # it parses; no decoder takes it
    # anywhere in the source, not only in the rectangle; and not where the part owns nothing
    with pytest.raises(ia.MpcError, match=": part 1: Invalid bitstream$") as e:
        ia.compose_container([cc.container(), bad], [(0, None, 0, 0), (1, (0, 0, 8, 8), 0, 0)], cc.W, cc.H)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM
    assert ia.compose_container([cc.container(), bad], [(1, (0, 0, 8, 8), 0, 0), (0, None, 0, 0)], cc.W, cc.H) == cc.container()


@pytest.mark.parametrize("case", range(len(cc.ARGUMENT_ERRORS)))
def test_argument_errors(ia, oracle, case):
    names, parts, width, height, word, who = cc.ARGUMENT_ERRORS[case]
    with pytest.raises(ia.MpcError) as e:
        ia.compose_container([cc.named(n) for n in names], parts, width, height)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT, str(e.value)
    assert word in str(e.value), str(e.value)
    if who:
        assert cc.text_of(e.value).startswith(who + ": "), str(e.value)


def test_pixels_and_no_sources_are_refused(ia, oracle):
    pixels = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ia.MpcError, match=": part 1: pixels need a device$") as e:
        ia.compose_container([cc.container()], [(0, None, 0, 0), (pixels, None, 0, 0)], cc.W, cc.H)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    with pytest.raises(ia.MpcError) as e:
        ia.compose_container([], [(pixels, None, 0, 0)], 8, 8)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT
