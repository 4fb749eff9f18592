"""Encode to a byte budget on the device (run with -m gpu): the depth profile kernel against mpc_distortion_device on cut counts and
against the oracle's decode of truncated containers, on encoder records and on the hand-made records of record_cases.py; the
allocation kernel against mpc_budget_allocate on the cases of budget_cases.py; and mpc_encode_image_budget[_device] end to end: the
search replayed with the public pieces alone, the bytes against the oracle's writeCompressed of the cut records, the reported errors
against numpy sums over the oracle's decode.  Both flavours, K in {1, 8, 32}; every equality is exact."""
import numpy as np
import pytest

import budget_cases as bc
import record_cases as rc

pytestmark = pytest.mark.gpu

FLAVOURS = (False, True)
KS = (1, 8, 32)
SHAPES = ((8, 8), (1, 1), (20, 12), (40, 40))           # one tile; one pixel; ragged both ways; 25 tiles: no multiple of the waves per workgroup


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


_contexts = {}


def _context(ia, K, fast=False):
    if (K, fast) not in _contexts:
        _contexts[K, fast] = ia.create_compression_context(K, 8, 3.5, device=0).set_fast(fast)
    return _contexts[K, fast]


@pytest.fixture(scope="module")
def photo(ia, mn_bytes):
    """The reference's own photograph (4928 x 3264), decoded from its .mn fixture by the product's decoder."""
    return np.ascontiguousarray(ia.decode_image(mn_bytes, _context(ia, 32)))


def _crop(photo, w, h, x=2003, y=1001):
    return np.ascontiguousarray(photo[y:y + h, x:x + w])


def _tile_sums(a, b):
    """per tile t = tx * tiles_y + ty the sum of squared differences of two [H, W, 3] frames"""
    H, W = a.shape[:2]
    d = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(axis=2)
    full = np.zeros((-(-H // 8) * 8, -(-W // 8) * 8), np.int64)
    full[:H, :W] = d
    return full.reshape(full.shape[0] // 8, 8, full.shape[1] // 8, 8).sum(axis=(1, 3)).T.reshape(-1)


class _Records:
    """whole-frame records on the host and on the device, beside the frame they belong to"""

    def __init__(self, counts, words, rgb):
        import torch
        self.counts, self.words, self.rgb = np.ascontiguousarray(counts, np.uint16), np.ascontiguousarray(words, np.uint32), rgb
        self.H, self.W = rgb.shape[:2]
        self.tiles, self.K = self.counts.shape[0], self.words.shape[2]
        self.d_counts = torch.from_numpy(self.counts.view(np.int16).copy()).cuda()
        self.d_choices = torch.from_numpy(self.words.view(np.int32).copy()).cuda()
        self.d_rgb = torch.from_numpy(np.array(rgb)).cuda()
        torch.cuda.synchronize()


def _encode(ctx, rgb):
    counts, choices, _e, _s = ctx.encode_tiles(rgb)
    return _Records(counts, np.ascontiguousarray(choices).view(np.uint32).reshape(counts.shape[0], 3, ctx.K), rgb)


def _profile(ctx, r, quant=None, check=True):
    import torch
    d_profile = torch.full((r.tiles, r.K + 1), -1, dtype=torch.int32, device="cuda")
    ctx.depth_profile_device(r.d_counts.data_ptr(), r.d_choices.data_ptr(), r.d_rgb.data_ptr(), r.W, r.H, d_profile.data_ptr(), quant=quant,
                             check=check)
    torch.cuda.synchronize()
    return d_profile.cpu().numpy().view(np.uint32).astype(np.int64), d_profile


def _distortion_at(ctx, r, n, quant=None):
    """mpc_distortion_device's tile sums with every count replaced by min(count, n)"""
    import torch
    d_cut = torch.from_numpy(np.minimum(r.counts, n).astype(np.uint16).view(np.int16)).cuda()
    d_sse = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_tiles = torch.full((r.tiles,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.distortion_device(d_cut.data_ptr(), r.d_choices.data_ptr(), r.d_rgb.data_ptr(), r.W, r.H, d_sse.data_ptr(), d_tiles.data_ptr(), quant=quant)
    torch.cuda.synchronize()
    return d_tiles.cpu().numpy().view(np.uint32).astype(np.int64)


def _profile_is_the_distortion(ctx, r, quant=None):
    P, _ = _profile(ctx, r, quant)
    assert P.shape == (r.tiles, r.K + 1)
    for n in range(r.K + 1):
        assert np.array_equal(P[:, n], _distortion_at(ctx, r, n, quant)), n
    deepest = np.minimum(r.counts.max(axis=1), r.K)
    for t in range(r.tiles):
        assert (P[t, deepest[t]:] == P[t, deepest[t]]).all()            # depths above a tile's largest count repeat the last value
    return P


# ---- 1. the profile ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("K", KS)
def test_profile_is_the_distortion_at_every_depth(ia, oracle, photo, K, fast):
    ctx = _context(ia, K, fast)
    for k, (w, h) in enumerate(SHAPES):
        for rgb in (oracle.synth_frame(w, h, 31 + k), _crop(photo, w, h, 2003 + 64 * k)):
            r = _encode(ctx, rgb)
            P = _profile_is_the_distortion(ctx, r)
            assert np.array_equal(P[:, 0], _tile_sums(rgb, np.zeros_like(rgb)))     # n = 0 is the all-black tile
    assert r.tiles == 25 and (np.diff(P, axis=1) != 0).any()


DEPTH_PARTS = [(K, fast, first) for K in KS for fast in FLAVOURS for first in range(1, K + 1, 8)]


@pytest.mark.parametrize("K,fast,first", DEPTH_PARTS)
def test_profile_is_the_error_of_the_truncated_container(ia, oracle, photo, K, fast, first):
    """one frame per flavour (the 40 x 40 crop), tile by tile against the oracle's decode of mpc_truncate_container(blob, n) for every
    n >= 1, eight depths a case: the oracle builds its dictionary for every decode"""
    ctx = _context(ia, K, fast)
    decode = oracle.decode_image_fast if fast else oracle.decode_image
    rgb = _crop(photo, 40, 40, 2003 + 64 * 3)
    P, _ = _profile(ctx, _encode(ctx, rgb))
    blob = ctx.encode_image(rgb)
    for n in range(first, min(first + 8, K + 1)):
        assert np.array_equal(P[:, n], _tile_sums(rgb, decode(ia.truncate_container(blob, n)))), n
    assert np.array_equal(P[:, 0], _tile_sums(rgb, np.zeros_like(rgb)))


# ---- 2. hand-made records ---------------------------------------------------------------------------------------------------------

def _hand_made(f, seed=0):
    rgb = np.random.default_rng(rc.SEED + seed).integers(0, 256, (f.H, f.W, 3)).astype(np.uint8)
    return _Records(f.counts, f.choices, rgb)


@pytest.mark.parametrize("fast", FLAVOURS)
def test_profile_of_hand_made_records(ia, oracle, fast):
    """repeats, dictionary edges, extreme coefficients, zero-coefficient unlocks: every list of wide_closed is prefix-consistent"""
    f = rc.frame("wide_closed")
    assert all(rc.closed(lst) for per_channel in f.records for lst in per_channel)
    ctx = _context(ia, f.K, fast)
    r = _hand_made(f)
    quant = f.quant.astype(np.float64)
    P = _profile_is_the_distortion(ctx, r, quant)
    decode = oracle.decode_image_fast if fast else oracle.decode_image
    for n in (1, 2, 3, 7, f.K):
        assert np.array_equal(P[:, n], _tile_sums(r.rgb, decode(ia.truncate_container(f.container, n)))), n


def _refused(ia, ctx, r, quant):
    with pytest.raises(ia.MpcError) as e:
        _profile(ctx, r, quant)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM and str(e.value).endswith("Invalid bitstream"), str(e.value)
    assert ctx.L.mpc_crop_records_check(ctx.h, None) == ia.api.MPC_OK          # read and cleared


@pytest.mark.parametrize("fast", FLAVOURS)
def test_records_that_are_not_prefix_consistent_are_refused(ia, fast):
    good = rc.frame("wide_closed")
    ctx = _context(ia, good.K, fast)
    r_good = _hand_made(good)
    quant = good.quant.astype(np.float64)
    want, _ = _profile(ctx, r_good, quant)
    # forward references
    for name in ("small", "wide"):
        f = rc.frame(name)
        assert any(not rc.closed(lst) for per_channel in f.records for lst in per_channel)
        c = _context(ia, f.K, fast)
        _refused(ia, c, _hand_made(f), f.quant.astype(np.float64))
    # one record outside its dictionary, in each channel and at the last step of a full list; the other tiles keep their profile
    for kind, ch, last in rc.bad_cases():
        b = rc.bad("wide_closed", kind, ch, last)
        r = _hand_made(b)
        _refused(ia, ctx, r, quant)
        P, _ = _profile(ctx, r, quant, check=False)
        assert ctx.L.mpc_crop_records_check(ctx.h, None) == ia.api.MPC_ERR_BITSTREAM
        others = np.arange(r.tiles) != b.bad_at[0]
        assert np.array_equal(P[others], want[others]), (kind, ch, last)
    # a count above K
    counts = good.counts.copy()
    counts[7, 1] = good.K + 1
    _refused(ia, ctx, _Records(counts, good.choices, r_good.rgb), quant)
    # the next call on the context is clean
    again, _ = _profile(ctx, r_good, quant)
    assert np.array_equal(again, want)


# ---- 3. the allocation kernel -----------------------------------------------------------------------------------------------------

CASES = bc.cases()


def _allocate_device(ctx, d_profile, d_counts, tiles, W, j):
    import torch
    d_depth = torch.full((tiles,), -1, dtype=torch.uint8, device="cuda")
    d_cut = torch.full((tiles, 3), -1, dtype=torch.int16, device="cuda")
    d_totals = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    ctx.budget_allocate_device(d_profile.data_ptr(), d_counts.data_ptr(), tiles, W, j, d_depth.data_ptr(), d_cut.data_ptr(), d_totals.data_ptr())
    torch.cuda.synchronize()
    return d_depth.cpu().numpy(), d_cut.cpu().numpy().view(np.uint16), [int(v) for v in d_totals.cpu().numpy().view(np.uint64)], d_cut, d_depth


@pytest.mark.parametrize("K", KS)
def test_allocation_kernel_is_the_host_function(ia, K):
    import torch
    ctx = _context(ia, K)
    mine = [c for c in CASES if c[1].shape[1] == K + 1]
    assert len(mine) >= 8
    for name, P, counts, W, js in mine:
        d_profile = torch.from_numpy(P.view(np.int32).copy()).cuda()
        d_counts = torch.from_numpy(counts.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        for j in js:
            depth, cut, totals, _, _ = _allocate_device(ctx, d_profile, d_counts, P.shape[0], W, j)
            want_depth, want_cut, want_totals = ia.budget_allocate(P, counts, W, j)
            assert np.array_equal(depth, want_depth) and np.array_equal(cut, want_cut), (name, j)
            assert totals == [int(v) for v in want_totals], (name, j)
            if j == 255:
                assert not depth.any() and not cut.any()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------

def _oracle_container(oracle, ctx, r, cut):
    """the oracle's writeCompressed of the records under the cut counts"""
    K = r.K
    codes = [[] for _ in range(6 * K)]
    for t in range(r.tiles):
        for ch in range(3):
            for i in range(int(cut[t, ch])):
                word = int(r.words[t, ch, i])
                codes[2 * K * ch + 2 * i].append(word & 0xFFFF)
                codes[2 * K * ch + 2 * i + 1].append(word >> 16)
    return oracle.write_compressed(dict(W=r.W, H=r.H, K=K, bs=8, quant=ctx.quant.astype(np.uint16), lengths=cut.reshape(-1),
                                        codes=[np.array(c, np.uint16) for c in codes]))


class _Replay:
    """the search of mpc_encode_image_budget with the public pieces alone: profile, weights, allocation, records -> container"""

    def __init__(self, ia, ctx, r, full):
        self.ia, self.ctx, self.r, self.full = ia, ctx, r, full
        self.weights = ia.budget_weights(ia.container_index(full))
        _, self.d_profile = _profile(ctx, r)
        self.made = {}

    def size(self, j):
        if j not in self.made:
            depth, cut, totals, d_cut, _ = _allocate_device(self.ctx, self.d_profile, self.r.d_counts, self.r.tiles, self.weights, j)
            blob = self.ctx.records_to_container_device(d_cut.data_ptr(), self.r.d_choices.data_ptr(), self.r.W, self.r.H)
            self.made[j] = (bytes(blob), depth, cut, totals)
        return self.made[j]

    def search(self, budget):
        """-> (lambda_index, probes, container, depth, cut counts, totals), or None where size(255) is above the budget"""
        if len(self.full) <= budget:
            return -1, 0, self.full, np.full(self.r.tiles, self.r.K, np.uint8), np.minimum(self.r.counts, self.r.K), None
        probes = 1
        if len(self.size(255)[0]) > budget:
            return None
        lo, hi = -1, 255
        while hi - lo > 1:
            mid = (lo + hi) // 2
            probes += 1
            if len(self.size(mid)[0]) <= budget:
                hi = mid
            else:
                lo = mid
        return (hi, probes) + self.size(hi)


def _sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", ("synthetic", "photograph"))
def test_budget_encode_end_to_end(ia, oracle, photo, kind, K, fast):
    ctx = _context(ia, K, fast)
    decode = oracle.decode_image_fast if fast else oracle.decode_image
    rgb = oracle.synth_frame(64, 48, 77) if kind == "synthetic" else _crop(photo, 131, 77)
    H, W = rgb.shape[:2]
    full = ctx.encode_image(rgb)
    r = _encode(ctx, rgb)
    replay = _Replay(ia, ctx, r, full)
    smallest = len(replay.size(255)[0])
    assert smallest < len(full)
    full_sse = _sse(rgb, decode(full))
    budgets = sorted({len(full), len(full) - 1, smallest} | {len(ia.truncate_container(full, m)) for m in (1, 2, 4)}, reverse=True)
    seen = set()
    for k, budget in enumerate(budgets):
        interval = (None, 0, 32)[k % 3]
        got = ctx.encode_image_budget(rgb, budget, index_interval=interval)
        want = replay.search(budget)
        assert want is not None, budget
        j, probes, blob, depth, cut, totals = want
        assert len(got.container) <= budget and probes <= 9
        assert (got.lambda_index, got.probes) == (j, probes), (budget, got)
        assert got.container == blob and np.array_equal(got.depth, depth), budget
        assert got.container == _oracle_container(oracle, ctx, r, cut), budget
        assert got.sse == _sse(rgb, decode(got.container)), budget
        assert got.full_sse == full_sse and got.full_bytes == len(full) and got.full_records == int(np.minimum(r.counts, K).sum())
        assert got.records == int(cut.sum())
        if totals is not None:
            assert got.sse == totals[0] and got.records == totals[2]
        if interval is None:
            assert got.index is None
        else:
            assert got.index == ia.container_index2(got.container, interval, ia.api.MPC_INDEX_EXPANDED), budget
        if budget == len(full):
            assert j == -1 and got.container == full and (got.depth == K).all()
        else:
            assert j >= 0 and got.sse >= 0 and got.records < got.full_records
            # what the result promises: hi fits, and lo -- the multiplier below, or the full container -- does not
            assert len(replay.size(j - 1)[0] if j > 0 else full) > budget
        seen.add(j)
        assert ctx.encode_image(rgb) == full                                    # the context is as it was
    assert -1 in seen and (K == 1 or len(seen) >= 3), seen
    # one byte below the smallest container there is
    with pytest.raises(ia.MpcError) as e:
        ctx.encode_image_budget(rgb, smallest - 1)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT and str(smallest - 1) in str(e.value) and str(smallest) in str(e.value), str(e.value)
    assert replay.search(smallest - 1) is None
    assert ctx.encode_image(rgb) == full
    assert len(ctx.encode_image_budget(rgb, smallest).container) == smallest


# ---- 5. the device form, refusals -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fast", FLAVOURS)
def test_device_form_equals_host_form_and_refusals(ia, oracle, photo, fast):
    import torch
    K = 8
    ctx = _context(ia, K, fast)
    rgb = _crop(photo, 131, 77, 900, 700)
    full = ctx.encode_image(rgb)
    d_rgb = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    made = {}
    for budget in (len(full), len(full) // 2, len(full) // 4):
        host = ctx.encode_image_budget(rgb, budget, index_interval=0)
        dev = ctx.encode_image_budget_device(d_rgb.data_ptr(), 131, 77, budget, index_interval=0)
        assert repr(host) == repr(dev) and host.container == dev.container and host.index == dev.index
        assert np.array_equal(host.depth, dev.depth) and len(host.container) <= budget
        made[budget] = host.container
    # a busy job slot: refused, and nothing of the call ran -- no pursuit was launched
    r = _encode(ctx, rgb)
    ctx.container_job_begin(3, r.d_counts.data_ptr(), r.d_choices.data_ptr(), 131, 77)
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    for call in (lambda: ctx.encode_image_budget(rgb, 1000), lambda: ctx.encode_image_budget_device(d_rgb.data_ptr(), 131, 77, 1000)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "slot 3 is busy" in str(e.value)
    assert ctx.read_kernel_timing()[1] == 0
    ctx.container_job_cancel(3)
    assert ctx.encode_image_budget(rgb, len(full) // 2).container == made[len(full) // 2]
    assert ctx.read_kernel_timing()[1] > 0
    ctx.kernel_timing(False)
    # the other refusals
    for bad in (lambda: ctx.encode_image_budget(rgb, 0), lambda: ctx.encode_image_budget(rgb, 1000, index_interval=7),
                lambda: ctx.encode_image_budget_device(0, 131, 77, 1000), lambda: ctx.encode_image_budget_device(d_rgb.data_ptr(), 0, 77, 1000)):
        with pytest.raises(ia.MpcError) as e:
            bad()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    host_only = ia.create_compression_context(K, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        host_only.encode_image_budget(rgb, 1000)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host_only.close()
    assert ctx.encode_image(rgb) == full

