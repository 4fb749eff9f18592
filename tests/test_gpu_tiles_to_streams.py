"""Stream assembly and its inverse on records that no pursuit emits (run with -m gpu): the hand-made cases of assembly_cases.py -- a lone
live tile in lane 63, in wave 15, as tile 1024 and as the last tile, waves and blocks alternately full and empty, an empty block between
live ones, an empty channel between two full ones, K = 5 across three blocks, 66 blocks, symbols over all of u16 and step-0
coefficients whose differences do not fit 16 bits -- through mp_stream_count / scan / scatter / dc (records to container, at once and
as a job in three steps), through the gather, the window ranks and the crop (container to records to container, whole and by
rectangle, with and without an index), and through the crop and the histogram kernel alone.  Every expected container is the ORACLE's
writeCompressed of the numpy model's streams, every expected record the model's; every equality is exact.  test_assembly_cases.py
shows on the CPU that these cases tell right kernels from twelve wrong ones.

One context per K, the default stream only.  No reconstruction, no pursuit, no pixels, no timing.  A count above K is handed to
the crop alone, whose behaviour include/mpcodec.h defines; on mpc_records_to_container_device the header is silent."""
import numpy as np
import pytest

import assembly_cases as ac
import stream_order as so

pytestmark = pytest.mark.gpu

NAMES = tuple(ac.CASES)
# NAMES shuffled (numpy's default_rng(1).permutation: a fixed order, written out).  The contexts are shared, so scratch grown for the 66 563 tiles of K = 2 is
# what the small frames of K = 2 behind it run in
ORDER = ("t1025_gap", "t66563", "t65_empty", "t1025", "t1023", "t1", "t63", "t2049", "t64", "t2049_lone", "t1024", "t65")
JOB_SLOTS = 6                                                       # MPC_JOB_SLOTS
ROUTES = (("version 1", False, 0), ("version 2", False, 0), ("version 2", True, 0), (None, False, 1))      # index, parse_all, route


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


_contexts = {}


def _context(ia, K):
    if K not in _contexts:
        _contexts[K] = ia.create_compression_context(K, 8, 3.5, device=0)
    return _contexts[K]


_uploaded = {}


def _upload(name):
    import torch
    if name not in _uploaded:
        c = ac.case(name)
        d_counts = torch.from_numpy(c.counts.view(np.int16).copy()).cuda()
        d_choices = torch.from_numpy(c.words.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        _uploaded[name] = (d_counts, d_choices)
    return _uploaded[name]


def _indexes(ia, blob):
    return {"version 1": ia.container_index(blob, 32), "version 2": ia.container_index(blob, 32, expanded=True), None: None}


# ---- records to container ---------------------------------------------------------------------------------------------------------

def test_the_order_is_a_shuffle_with_small_frames_behind_the_big_one():
    assert ORDER == tuple(NAMES[i] for i in np.random.default_rng(1).permutation(len(NAMES)))
    behind = ORDER[ORDER.index(ac.BIG) + 1:]
    assert any(ac.case(n).K == ac.case(ac.BIG).K and ac.case(n).tiles < 100 for n in behind)


@pytest.mark.parametrize("name", ORDER)
def test_records_to_container(ia, oracle, name):
    c = ac.case(name)
    ctx = _context(ia, c.K)
    want = ac.container(oracle, name)
    d_counts, d_choices = _upload(name)
    quant = c.quant.astype(np.float64)
    assert bytes(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), c.W, c.H, quant=quant)) == want
    slot = 1 + ORDER.index(name) % (JOB_SLOTS - 1)                  # never slot 0
    ctx.container_job_begin(slot, d_counts.data_ptr(), d_choices.data_ptr(), c.W, c.H, quant=quant)
    ctx.container_job_tables(slot)
    assert bytes(ctx.container_job_collect(slot)) == want, slot
    assert bytes(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), c.W, c.H, quant=quant)) == want      # and again


def test_the_host_entropy_route_on_the_wild_cases(ia, oracle, monkeypatch):
    """MPC_HOST_ENTROPY=1 is read when a context is made: the assembled symbols cross to the host as they are"""
    monkeypatch.setenv("MPC_HOST_ENTROPY", "1")
    made = {}
    for name in ac.WILD:
        c = ac.case(name)
        if c.K not in made:
            made[c.K] = ia.create_compression_context(c.K, 8, 3.5, device=0)
        d_counts, d_choices = _upload(name)
        got = made[c.K].records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), c.W, c.H, quant=c.quant.astype(np.float64))
        assert bytes(got) == ac.container(oracle, name), name
    for ctx in made.values():
        ctx.close()


# ---- container to records to container: the tame cases ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.TAME)
def test_the_whole_frame_comes_back_byte_for_byte(ia, oracle, name):
    c = ac.case(name)
    ctx = _context(ia, c.K)
    blob = ac.container(oracle, name)
    indexes = _indexes(ia, blob)
    for which, parse_all, route in ROUTES:
        got, routes = ctx.transcode_views([blob], [indexes[which]], [(None, 0, 0)], parse_all)
        assert routes == [route], (which, parse_all, routes)
        assert bytes(got[0]) == blob, (which, parse_all)


@pytest.mark.parametrize("name", tuple(ac.RECTS))
def test_rectangles(ia, oracle, name):
    """first and last tiles on 63 | 64 and 1023 | 1024, inside block 1, one tile column, the last tile alone: the window ranks with
    aligned and unaligned t0 and with t1 == tiles, the windowed gather, the crop, the scatter"""
    c = ac.case(name)
    ctx = _context(ia, c.K)
    blob = ac.container(oracle, name)
    indexes = _indexes(ia, blob)
    rects = ac.RECTS[name]
    views = [(c.rect_pixels(grid), 0, 0) for grid in rects.values()]
    want = [ac.crop_container(oracle, name, grid, c.K) for grid in rects.values()]
    n = len(views)
    for which, parse_all, route in ROUTES:
        got, routes = ctx.transcode_views([blob] * n, [indexes[which]] * n, views, parse_all)
        assert routes == [route] * n, (which, parse_all, routes)
        for what, g, w in zip(rects, got, want):
            assert bytes(g) == w, (what, which, parse_all)


@pytest.mark.parametrize("name", tuple(ac.STEP_CUTS))
def test_step_cuts(ia, oracle, name):
    c = ac.case(name)
    ctx = _context(ia, c.K)
    blob = ac.container(oracle, name)
    indexes = _indexes(ia, blob)
    assert ac.STEP_CUTS[name] == (1, c.K - 1, c.K)
    grids = [None, ac.RECTS[name]["first_64"]]
    views = [(c.rect_pixels(grid) if grid else None, steps, 0) for grid in grids for steps in ac.STEP_CUTS[name]]
    want = [ac.crop_container(oracle, name, grid, steps) for grid in grids for steps in ac.STEP_CUTS[name]]
    n = len(views)
    for which, parse_all, route in ROUTES:
        got, routes = ctx.transcode_views([blob] * n, [indexes[which]] * n, views, parse_all)
        assert routes == [route] * n, (which, parse_all, routes)
        for view, g, w in zip(views, got, want):
            assert bytes(g) == w, (view, which, parse_all)


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------

def _crop_on_device(ia, ctx, c, d_counts, d_choices, grid, steps):
    """mp_crop_records_kernel into poisoned buffers, the check behind it -> (counts, words, what the check raised)"""
    import torch
    n = (grid[1] - grid[0]) * (grid[3] - grid[2])
    out_counts = torch.full((n, 3), 0x5A5A, dtype=torch.int16, device="cuda")
    out_words = torch.full((n, 3, c.K), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    error = None
    try:
        ctx.crop_records_device(d_counts.data_ptr(), d_choices.data_ptr(), c.W, c.H, c.rect_pixels(grid), steps, out_counts.data_ptr(),
                                out_words.data_ptr(), check=True)
    except ia.MpcError as e:
        error = e
    torch.cuda.synchronize()
    return out_counts.cpu().numpy().view(np.uint16), out_words.cpu().numpy().view(np.uint32), error


@pytest.mark.parametrize("name", tuple(ac.RECTS))
def test_the_crop_kernel_is_the_models_crop(ia, name):
    """on the records as uploaded, garbage behind every count: the dead steps come out zero, and the check stays silent"""
    c = ac.case(name)
    ctx = _context(ia, c.K)
    d_counts, d_choices = _upload(name)
    whole = (0, c.tiles_x, 0, c.tiles_y)
    for grid in list(ac.RECTS[name].values()) + [whole]:
        for steps in (0, 1, c.K - 1):
            got = _crop_on_device(ia, ctx, c, d_counts, d_choices, grid, steps)
            want = ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, grid, steps or c.K)
            assert got[2] is None, (grid, steps, str(got[2]))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (grid, steps)


def test_the_crop_kernel_uses_a_count_above_k_as_k(ia):
    import torch
    c = ac.case(ac.ABOVE_K[0])
    at = ac.ABOVE_K[4]
    ctx = _context(ia, c.K)
    d_counts = torch.from_numpy(c.counts.view(np.int16).copy()).cuda()
    _, d_choices = _upload("t2049")                                  # the same words
    assert np.array_equal(c.words, ac.case("t2049").words) and c.counts[at, 0] == c.K + 1
    tx = at // c.tiles_y
    around, away = (tx - 3, tx + 7, 0, c.tiles_y), (tx + 7, tx + 9, 0, c.tiles_y)
    got = _crop_on_device(ia, ctx, c, d_counts, d_choices, around, 0)
    error = got[2]
    assert error is not None and error.status == ia.api.MPC_ERR_BITSTREAM and str(error).endswith("Invalid bitstream"), str(error)
    want = ac.crop(np.minimum(c.counts, c.K), c.words, c.tiles_x, c.tiles_y, around, c.K)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].max() == c.K
    # a rectangle beside the tile never looks at it, and the check has cleared the word
    got = _crop_on_device(ia, ctx, c, d_counts, d_choices, away, 0)
    want = ac.crop(c.counts, c.words, c.tiles_x, c.tiles_y, away, c.K)
    assert got[2] is None and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", ("t1025_gap", "t63"))
def test_the_histogram_kernel_leaves_symbols_beyond_its_table_out(ia, name):
    import torch
    c = ac.case(name)
    assert c.family == "wild"
    ctx = _context(ia, c.K)
    d_counts, d_choices = _upload(name)
    bins = 8192
    d_hist = torch.zeros((1 + 6 * c.K, bins), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.histogram_device(d_counts.data_ptr(), d_choices.data_ptr(), c.tiles, d_hist.data_ptr())
    torch.cuda.synchronize()
    counts, words = np.array(c.counts), np.array(c.words)
    every = so.histogram(counts, words, c.K, bins=65536)
    assert every[1:, bins:].sum() > every[1:, :bins].sum() > 0          # most live symbols lie beyond the table, some inside
    assert np.array_equal(d_hist.cpu().numpy().view(np.uint32), every[:, :bins])
