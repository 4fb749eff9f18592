"""The hand-made records of tests/assembly_cases.py, checked on the CPU: every case is what it is for, the host's stream assembly and
transcode give the oracle's bytes of the numpy model's streams, the oracle reads those bytes back as what was put in, and every
mistake the kernel-shaped restatement can be switched to changes what a container holds.  test_gpu_tiles_to_streams.py relies on all
of it: a case that lost a property would still pass there and test nothing.  Every expected byte is the oracle's writeCompressed of
the model's streams; the restatement only shows that the cases discriminate."""
import numpy as np
import pytest

import assembly_cases as ac
import stream_order

NAMES = tuple(ac.CASES)
BY_SIZE = sorted(NAMES, key=lambda n: (ac.case(n).tiles, ac.case(n).K))
# per mutant the smallest case (by tiles, then K) that shows it; no smaller one does.  no_clamp needs a count above K: `above_k` alone
SMALLEST = {
    "rank_per_wave": "t65",                     # the first frame with live tiles in two waves of one stream
    "no_block_offset": "t1025_gap",             # ... in two blocks
    "inclusive_scan": "t1",
    "carry_lost": "t66563",                     # the only frame of more than 64 blocks
    "stale_wave_live": "t65",
    "dc_prev_across": "t63",                    # t1's step-0 coefficients are 0: a carried 0 is no mistake
    "dc_clamp": "t63",
    "swap_halves": "t1",
    "dc_ch0_only": "t63",
    "no_clamp": ac.ABOVE_K[0],
}


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _coded_bytes(ia, c, coded):
    """the container of streams that are already differenced, by the host coder: for telling mutants apart only"""
    return ia.assemble_symbol_streams(c.W, c.H, c.K, 8, c.quant.astype(np.float64), c.counts, coded)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_is_what_it_is_for(name):
    ac.check(name)


def test_the_families_and_sizes_are_all_there():
    ac.check_families()
    c = ac.case(ac.ABOVE_K[0])
    assert c.counts.max() == c.K + 1 and (c.counts > c.K).sum() == 1 and c.counts[ac.ABOVE_K[4], 0] == c.K + 1 and c.tiles > 2 * ac.BLOCK


@pytest.mark.parametrize("name", NAMES)
def test_host_assembly_gives_the_oracles_bytes(ia, oracle, name):
    c = ac.case(name)
    want = ac.container(oracle, name)
    assert bytes(ia.assemble_streams(c.W, c.H, c.K, 8, c.quant.astype(np.float64), c.counts, c.words)) == want
    # the restatement in the kernels' shape is the model, and its differenced streams are what the container holds
    coded = ac.coded_streams(c.counts, c.words, c.K)
    assert _same(coded, ac.code(ac.streams(c.counts, c.words, c.K), c.K))
    assert bytes(_coded_bytes(ia, c, coded)) == want


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_reads_back_what_was_put_in(oracle, name):
    c = ac.case(name)
    st = oracle.read_compressed(ac.container(oracle, name))
    held = ac.streams(c.counts, c.words, c.K)
    assert (st["W"], st["H"], st["K"], st["bs"]) == (c.W, c.H, c.K, 8) and np.array_equal(st["quant"], c.quant)
    assert np.array_equal(st["lengths"], c.counts.reshape(-1))
    assert [len(x) for x in st["codes"]] == [len(x) for x in held]
    # a wild step-0 coefficient stream comes back as the sum of its truncated differences; everything else as it went in
    back = ac.read_back(held, c.K)
    assert _same([np.asarray(x, np.uint16) for x in st["codes"]], back)
    dc = [2 * c.K * ch + 1 for ch in range(3)]
    assert all(np.array_equal(back[i], held[i]) for i in range(6 * c.K) if i not in dc)
    if c.family == "tame":
        assert _same(back, held)
    elif max(len(held[i]) for i in dc) >= 16:
        assert any(not np.array_equal(back[i], held[i]) for i in dc)


def _views(name):
    c = ac.case(name)
    views = [(None, 0)] + [(grid, 0) for grid in ac.RECTS.get(name, {}).values()]
    for steps in ac.STEP_CUTS.get(name, ()):
        views += [(None, steps), (ac.RECTS[name]["first_64"], steps)]
    return c, views


@pytest.mark.parametrize("name", ac.TAME)
def test_host_transcode_gives_the_oracles_bytes_of_the_crop(ia, oracle, name):
    c, views = _views(name)
    blob = ac.container(oracle, name)
    for grid, steps in views:
        got = ia.transcode_container(blob, (c.rect_pixels(grid) if grid else None, steps, 0))
        assert bytes(got) == ac.crop_container(oracle, name, grid, steps or c.K), (name, grid, steps)
    assert ac.crop_container(oracle, name, None, c.K) == blob       # the whole frame, uncut: the source itself
    if name in ac.STEP_CUTS:
        assert ac.STEP_CUTS[name] == (1, c.K - 1, c.K)


@pytest.mark.parametrize("name", ac.TAME)
def test_the_tame_containers_have_usable_indexes(ia, oracle, name):
    """the device test expects route 0 with either index: neither may say "serial only" """
    blob = ac.container(oracle, name)
    for expanded in (False, True):
        info = ia.index_info(ia.container_index(blob, 32, expanded=expanded))
        assert not info["serial_only"] and info["K"] == ac.case(name).K, (name, expanded)


@pytest.mark.parametrize("name", ("t1025_gap", "t63"))
def test_the_histogram_cases_reach_beyond_the_table(name):
    """the cases the device test gives the histogram kernel: most live symbols are 8192 or more, some are less"""
    c = ac.case(name)
    every = stream_order.histogram(np.array(c.counts), np.array(c.words), c.K, bins=65536)
    assert c.family == "wild" and every[1:, 8192:].sum() > every[1:, :8192].sum() > 0
    assert every[0].sum() == 3 * c.tiles and every[0, c.K + 1:].sum() == 0


@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_every_mutant_changes_a_container(ia, oracle, mutant):
    name = SMALLEST[mutant]
    c = ac.case(name)
    right, wrong = ac.coded_streams(c.counts, c.words, c.K), ac.coded_streams(c.counts, c.words, c.K, mutant)
    assert not _same(wrong, right)
    if mutant == "no_clamp":                    # the tile is not counted: a stream one symbol short of what the lengths say, no container at all
        assert sum(len(x) for x in wrong) < sum(len(x) for x in right)
    else:
        assert [len(x) for x in wrong] == [len(x) for x in right]
        assert bytes(_coded_bytes(ia, c, wrong)) != bytes(_coded_bytes(ia, c, right))
    for smaller in BY_SIZE[:BY_SIZE.index(name)] if name in BY_SIZE else [n for n in BY_SIZE if n != ac.BIG]:
        s = ac.case(smaller)
        assert _same(ac.coded_streams(s.counts, s.words, s.K, mutant), ac.coded_streams(s.counts, s.words, s.K)), (mutant, smaller)


def test_every_crop_mutant_changes_records_or_bytes(oracle):
    c = ac.case("t1025")
    grid = ac.RECTS["t1025"]["first_64"]
    counts, words = ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, grid, c.K)
    # dead steps kept: the records differ; no container can show it, which is why the device test compares the crop's records
    kept_counts, kept_words = ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, grid, c.K, "crop_keeps_dead")
    assert np.array_equal(kept_counts, counts) and (kept_words != words).any()
    assert _same(ac.streams(kept_counts, kept_words, c.K), ac.streams(counts, words, c.K))
    cut_counts, cut_words = ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, grid, 1, "crop_keeps_dead")
    assert (cut_words[:, :, 1:] != 0).any() and not ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, grid, 1)[1][:, :, 1:].any()
    # tiles taken y-outer: the bytes differ, in every rectangle of more than one row and column
    for name, rects in ac.RECTS.items():
        f = ac.case(name)
        for what, g in rects.items():
            turned = ac.crop(f.counts, f.words, f.tiles_x, f.tiles_y, g, f.K, "crop_y_outer")
            _, _, w, h = f.rect_pixels(g)
            differs = ac.oracle_bytes(oracle, w, h, f.K, f.quant, *turned) != ac.crop_container(oracle, name, g, f.K)
            assert differs == (g[1] - g[0] > 1 and g[3] - g[2] > 1), (name, what)


def test_a_count_above_k(ia, oracle):
    """What include/mpcodec.h says of a count above K, asserted where it says something:
      mpc_transcode_container   "a length above K anywhere in the frame is MPC_ERR_BITSTREAM "Invalid bitstream""
      mpc_crop_records_device   "a count above K is used as K" (the model's crop does that; the device test holds the kernel to it)
    On mpc_assemble_streams and mpc_records_to_container_device the header is silent: nothing is asserted, and no test hands
    either a count above K."""
    c = ac.case(ac.ABOVE_K[0])
    K = c.K
    bad = ac.oracle_bytes(oracle, c.W, c.H, K, c.quant, c.counts, c.words)
    for view in ((None, 0, 0), ((0, 0, 8, 8), 1, 0)):
        with pytest.raises(ia.MpcError) as e:
            ia.transcode_container(bad, view)
        assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid bitstream"), str(e.value)
    whole = (0, c.tiles_x, 0, c.tiles_y)
    used_as_k = ac.crop(np.minimum(c.counts, K), c.words, c.tiles_x, c.tiles_y, whole, K)
    got = ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, whole, K)
    assert np.array_equal(got[0], used_as_k[0]) and np.array_equal(got[1], used_as_k[1]) and got[0].max() == K
