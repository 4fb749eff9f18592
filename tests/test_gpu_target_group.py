"""A group of frames to one byte budget or one quality on the device (run with -m gpu): the two group kernels against
mpc_budget_allocate_group and mpc_budget_sweep_group on every case of group_cases.py, with and without a map; both device pieces' stream
contract through the harness of stream_order.py and their refusal of a capturing stream; mpc_encode_images_budget[_device] and
mpc_encode_images_quality[_device] end to end -- the budget call replayed with the single-frame public pieces alone, the quality call
against the replayed sweep, pick and allocation, every frame's reported error against the oracle's decode -- one frame against the
single-frame calls, a budget the full containers fit against mpc_encode_images, the device forms against the host forms, a neutral map
against none, the refusals, and mpc_encode_images unchanged afterwards.  Every equality is exact.

The file's name sorts it behind test_gpu_stream_order.py for the reason given at the top of test_gpu_target_quality.py."""
import math

import numpy as np
import pytest

import budget_cases as bc
import group_cases as gc
import stream_order as so

pytestmark = pytest.mark.gpu

FLAVOURS = (False, True)
W, H = 64, 48
TILES = (W // 8) * (H // 8)


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
def group_frames(ia, oracle, mn_bytes):
    """frames of differing content, 64 x 48: a synthetic frame, a flat one, a crop of the reference's photograph (decoded from its .mn
    fixture by the product's decoder), a second synthetic one"""
    photo = ia.decode_image(mn_bytes, _context(ia, 32))
    return [oracle.synth_frame(W, H, 77), np.full((H, W, 3), 90, np.uint8), np.ascontiguousarray(photo[1001:1001 + H, 2003:2003 + W]),
            oracle.synth_frame(W, H, 78)]


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------

CASES = gc.cases()


def _to_device(torch, P, counts, E):
    d = (torch.from_numpy(P.view(np.int32).copy()).cuda(), torch.from_numpy(counts.view(np.int16).copy()).cuda(), torch.from_numpy(E.copy()).cuda())
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("K", gc.KS)
def test_group_kernels_are_the_host_functions(ia, K):
    import torch
    ctx = _context(ia, K)
    S = torch.cuda.Stream()
    mine = [c for c in CASES if c[1].shape[2] == K + 1]
    assert len(mine) == len(gc.FRAME_COUNTS) * len(gc.TILE_COUNTS)
    for name, P, counts, E, Wt, js in mine:
        F, T = P.shape[:2]
        d_profile, d_counts, d_map = _to_device(torch, P, counts, E)
        for label, e, d_e in (("map", E, d_map.data_ptr()), ("no map", None, 0)):
            for j in js:
                d_depth = torch.full((F, T), 0xEE, dtype=torch.uint8, device="cuda")               # poison: every byte is written
                d_cut = torch.full((F, T, 3), -1, dtype=torch.int16, device="cuda")
                d_totals = torch.full((F, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")  # garbage: the call zeroes it
                torch.cuda.synchronize()
                ctx.budget_allocate_group_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e, F, T, Wt, j, d_depth.data_ptr(), d_cut.data_ptr(),
                                                 d_totals.data_ptr(), stream=S.cuda_stream)
                S.synchronize()
                depth, cut, totals = ia.budget_allocate_group(P, counts, e, Wt, j)
                assert np.array_equal(d_depth.cpu().numpy(), depth) and np.array_equal(d_cut.cpu().numpy().view(np.uint16), cut), (name, label, j)
                assert np.array_equal(d_totals.cpu().numpy().view(np.uint64), totals), (name, label, j)
                if j == 255:
                    assert not depth.any() and not cut.any()
            d_sweep = torch.full((gc.LAMBDAS, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ctx.budget_sweep_group_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e, F, T, Wt, d_sweep.data_ptr(), stream=S.cuda_stream)
            S.synchronize()
            got, want = d_sweep.cpu().numpy().view(np.uint64), ia.budget_sweep_group(P, counts, e, Wt)
            assert got.shape == (gc.LAMBDAS, 3) and np.array_equal(got, want), (name, label, int((got != want).sum()))


def test_group_kernels_beyond_one_trip_of_a_workgroup(ia):
    """more tiles a frame than the allocation's and the sweep's grids take in one round, so that a workgroup's loop goes round inside
    its frame: 9 frames of 4096 * 4 + 3 tiles at K = 1 (the sweep's cap is shared by the frames of a launch)"""
    import torch
    K, F, T = 1, 9, 4096 * 4 + 3
    ctx = _context(ia, K)
    rng = np.random.default_rng(5)
    counts = rng.integers(0, K + 2, (F, T, 3)).astype(np.uint16)
    P = bc._consistent_profile(rng, np.minimum(counts.reshape(-1, 3), K), K, monotone=False).reshape(F, T, K + 1)
    E = rng.integers(0, 80, (F, T)).astype(np.uint8)
    Wt = gc.octave_weights(rng, F, K)
    d_profile, d_counts, d_map = _to_device(torch, P, counts, E)
    for e, d_e in ((E, d_map.data_ptr()), (None, 0)):
        d_depth = torch.full((F, T), 0xEE, dtype=torch.uint8, device="cuda")
        d_cut = torch.full((F, T, 3), -1, dtype=torch.int16, device="cuda")
        d_totals = torch.full((F, 3), -1, dtype=torch.int64, device="cuda")
        d_sweep = torch.full((gc.LAMBDAS, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.budget_allocate_group_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e, F, T, Wt, 90, d_depth.data_ptr(), d_cut.data_ptr(), d_totals.data_ptr())
        ctx.budget_sweep_group_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e, F, T, Wt, d_sweep.data_ptr())
        torch.cuda.synchronize()
        depth, cut, totals = ia.budget_allocate_group(P, counts, e, Wt, 90)
        assert np.array_equal(d_depth.cpu().numpy(), depth) and np.array_equal(d_cut.cpu().numpy().view(np.uint16), cut)
        assert np.array_equal(d_totals.cpu().numpy().view(np.uint64), totals)
        assert np.array_equal(d_sweep.cpu().numpy().view(np.uint64), ia.budget_sweep_group(P, counts, e, Wt))


# ---- 2. the stream contract -------------------------------------------------------------------------------------------------------

def _order_inputs(K, F, T):
    def inputs(seed):
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, K + 1, (F, T, 3)).astype(np.uint16)
        return bc._consistent_profile(rng, counts.reshape(-1, 3), K, monotone=False).reshape(F, T, K + 1), counts

    return inputs(41), inputs(42), gc.octave_weights(np.random.default_rng(43), F, K)


def test_group_device_pieces_are_ordered_on_the_callers_stream_and_asynchronous(ia):
    import torch
    K, F, T, j = 8, 9, 375, 100
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    (pa, ca), (pb, cb), weights = _order_inputs(K, F, T)
    want_sweep, other = ia.budget_sweep_group(pa, ca, None, weights), ia.budget_sweep_group(pb, cb, None, weights)
    depth, cut, totals = ia.budget_allocate_group(pa, ca, None, weights, j)
    assert not np.array_equal(want_sweep, other) and not np.array_equal(depth, ia.budget_allocate_group(pb, cb, None, weights, j)[0])

    def sweep(b):
        ctx.budget_sweep_group_device(b.ptr("profile"), b.ptr("counts"), 0, F, T, weights, b.ptr("totals"), stream=b.stream)
        b.probe()

    def allocate(b):
        ctx.budget_allocate_group_device(b.ptr("profile"), b.ptr("counts"), 0, F, T, weights, j, b.ptr("depth"), b.ptr("cut"), b.ptr("totals"), stream=b.stream)
        b.probe()

    S = torch.cuda.Stream()
    cpm = so.cycles_per_ms(torch)
    try:
        inputs = {"profile": (pa, pb), "counts": (ca, cb)}
        for label, call, outputs in (("budget_sweep_group_device", sweep, {"totals": want_sweep}),
                                     ("budget_allocate_group_device", allocate, {"depth": depth, "cut": cut, "totals": totals})):
            _, _, warm = so.behind_delay(torch, S, call, inputs, outputs, 1000)
            delay = so.delay_ms_for(warm["host_ms"])
            got, _, info = so.behind_delay(torch, S, call, inputs, outputs, delay * cpm)
            print(f"{label}: warm-up enqueue {warm['host_ms']:.2f} ms, delay {delay:.0f} ms, enqueue behind the delay {info['host_ms']:.2f} ms, "
                  f"delay still running at return: {info['running']}")
            for name, want in outputs.items():
                assert np.array_equal(got[name], want), (label, name, int((got[name] != want).sum()))
            assert info["running"], f"{label} returned only after the stream had drained"
    finally:
        ctx.close()


def test_group_device_pieces_refuse_a_capturing_stream_on_a_context_that_has_made_no_call(ia):
    import torch
    K, F, T = 8, 3, 375
    fresh = ia.create_compression_context(K, 8, 3.5, device=0)
    try:
        S = torch.cuda.Stream()
        d = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda")
        marker = torch.zeros(16, dtype=torch.int32, device="cuda")
        weights = np.full((F, 3, K), 1000, np.uint32)
        p = d.data_ptr()
        calls = (lambda s=0, frames=F, tiles=T, a=p, b=p, c=p: fresh.budget_sweep_group_device(a or None, b or None, 0, frames, tiles, weights[:max(min(frames, F), 1)], c or None, stream=s),
                 lambda s=0, frames=F, tiles=T, a=p, b=p, c=p: fresh.budget_allocate_group_device(a or None, b or None, 0, frames, tiles, weights[:max(min(frames, F), 1)], 7, p, p, c or None, stream=s))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=S):
            marker.add_(1)
            for call in calls:
                with pytest.raises(ia.MpcError) as e:
                    call(torch.cuda.current_stream().cuda_stream)
                assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "captured" in str(e.value), str(e.value)
            marker.add_(1)
        torch.cuda.synchronize()
        assert int(marker[0]) == 0                                  # the capture ended cleanly and nothing ran
        graph.replay()
        torch.cuda.synchronize()
        assert int(marker[0]) == 2 and not d.cpu().numpy().any()    # the caller's two kernels and nothing else
        # the other refusals: nothing enqueued either
        for call in calls:
            for kw in (dict(a=0), dict(b=0), dict(c=0), dict(tiles=0), dict(tiles=-5), dict(tiles=(1 << 31) // 9 + 1), dict(frames=0), dict(frames=65),
                       dict(frames=-1)):
                with pytest.raises(ia.MpcError) as e:
                    call(**kw)
                assert e.value.status == ia.api.MPC_ERR_ARGUMENT, kw
        with pytest.raises(ia.MpcError) as e:
            fresh.budget_allocate_group_device(p, p, 0, F, T, weights, 256, p, p, p)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
        torch.cuda.synchronize()
        assert not d.cpu().numpy().any()
    finally:
        fresh.close()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------

def _floor(ctx, frames):
    """the bytes of the smallest containers there are: every tile cut to nothing, the last multiplier's allocation"""
    cut = ctx.encode_images_quality(frames, max_sse=1 << 63)
    assert cut.info.lambda_index == 255 and cut.info.records == 0
    return cut.size


def _sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


_decoded = {}


def _once(decode):
    """the oracle's decode, every container once: the tests of this file meet the same containers again and again"""
    def cached(blob):
        key = (decode.__name__, bytes(blob))
        if key not in _decoded:
            _decoded[key] = decode(blob)
        return _decoded[key]

    return cached


class _Frame:
    """one frame of the group with the single-frame public pieces alone: encode_tiles_device, records_to_container_device,
    container_index, budget_weights, depth_profile_device, budget_allocate_device, budget_sweep_device"""

    def __init__(self, ia, ctx, rgb):
        import torch
        self.ia, self.ctx, self.torch, self.rgb, self.K = ia, ctx, torch, rgb, ctx.K
        self.d_rgb = torch.from_numpy(rgb).cuda()
        self.d_counts = torch.zeros((TILES, 3), dtype=torch.int16, device="cuda")
        self.d_choices = torch.zeros((TILES, 3, self.K), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.encode_tiles_device(self.d_rgb.data_ptr(), W, H, 3 * W, 0, H // 8, self.d_counts.data_ptr(), self.d_choices.data_ptr())
        torch.cuda.synchronize()
        self.full = bytes(ctx.records_to_container_device(self.d_counts.data_ptr(), self.d_choices.data_ptr(), W, H))
        self.weights = ia.budget_weights(ia.container_index(self.full))
        self.d_profile = torch.full((TILES, self.K + 1), -1, dtype=torch.int32, device="cuda")
        ctx.depth_profile_device(self.d_counts.data_ptr(), self.d_choices.data_ptr(), self.d_rgb.data_ptr(), W, H, self.d_profile.data_ptr())
        d_totals = torch.full((gc.LAMBDAS, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.budget_sweep_device(self.d_profile.data_ptr(), self.d_counts.data_ptr(), TILES, self.weights, d_totals.data_ptr())
        torch.cuda.synchronize()
        self.S = d_totals.cpu().numpy().view(np.uint64)
        self.records = int(np.minimum(self.d_counts.cpu().numpy().view(np.uint16), self.K).sum())
        self.made = {}

    def at(self, j):
        """-> (container, depth, totals) of the frame's allocation at multiplier j"""
        if j not in self.made:
            torch = self.torch
            d_depth = torch.full((TILES,), -1, dtype=torch.uint8, device="cuda")
            d_cut = torch.full((TILES, 3), -1, dtype=torch.int16, device="cuda")
            d_totals = torch.full((3,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            self.ctx.budget_allocate_device(self.d_profile.data_ptr(), self.d_counts.data_ptr(), TILES, self.weights, j, d_depth.data_ptr(),
                                            d_cut.data_ptr(), d_totals.data_ptr())
            torch.cuda.synchronize()
            blob = bytes(self.ctx.records_to_container_device(d_cut.data_ptr(), self.d_choices.data_ptr(), W, H))
            self.made[j] = (blob, d_depth.cpu().numpy(), [int(v) for v in d_totals.cpu().numpy().view(np.uint64)])
        return self.made[j]


class _Replay:
    """the group calls from their frames' replays: size(j) the sum of the frames' containers at j, the search of test_gpu_budget.py's
    _Replay over it, the sweep the sum of the frames' sweeps"""

    def __init__(self, ia, ctx, frames):
        self.frames = [_Frame(ia, ctx, rgb) for rgb in frames]
        self.K = ctx.K
        self.full = sum(len(f.full) for f in self.frames)
        self.S = sum(f.S for f in self.frames)
        self.D = [int(v) for v in self.S[:, 0]]

    def size(self, j):
        return sum(len(f.at(j)[0]) for f in self.frames)

    def search(self, budget):
        """-> (lambda_index, probes), or None where size(255) is above the budget"""
        if self.full <= budget:
            return -1, 0
        probes = 1
        if self.size(255) > budget:
            return None
        lo, hi = -1, 255
        while hi - lo > 1:
            mid = (lo + hi) // 2
            probes += 1
            if self.size(mid) <= budget:
                hi = mid
            else:
                lo = mid
        return hi, probes

    def at(self, j):
        """[(container, depth, totals)] per frame; j = -1: the full containers, every depth K"""
        if j < 0:
            return [(f.full, np.full(TILES, self.K, np.uint8), None) for f in self.frames]
        return [f.at(j) for f in self.frames]


_replays = {}


def _replay(ia, ctx, frames, K, fast, n):
    if (K, fast, n) not in _replays:
        _replays[K, fast, n] = _Replay(ia, ctx, frames[:n])
    return _replays[K, fast, n]


def _check_frames(ia, got, want, frames, decode, interval):
    """every frame of a group result against its replay: container, depth, index, the reported error against the oracle's decode"""
    for f, (blob, depth, totals) in enumerate(want):
        assert got[f].container == blob and np.array_equal(got[f].depth, depth), f
        assert got[f].sse == _sse(frames[f], decode(got[f].container)), f
        if totals is not None:
            assert got[f].sse == totals[0] and got[f].records == totals[2], f
        if interval is None:
            assert got[f].index is None
        else:
            assert got[f].index == ia.container_index2(got[f].container, interval, ia.api.MPC_INDEX_EXPANDED), f


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("K", gc.KS)
@pytest.mark.parametrize("n", (1, 2, 3))
def test_group_budget_encode_end_to_end(ia, oracle, group_frames, n, K, fast):
    import torch
    ctx = _context(ia, K, fast)
    decode = _once(oracle.decode_image_fast if fast else oracle.decode_image)
    frames = group_frames[:n]
    fulls = ctx.encode_images(frames)
    replay = _replay(ia, ctx, group_frames, K, fast, n)
    assert [f.full for f in replay.frames] == fulls
    d_frames = [torch.from_numpy(rgb).cuda() for rgb in frames]
    torch.cuda.synchronize()
    smallest = replay.size(255)
    assert smallest < replay.full
    seen = set()
    for k, budget in enumerate((replay.full, replay.full - 1, replay.full // 2, replay.full // 4, smallest)):
        interval = (None, 0, 32)[k % 3]
        want = replay.search(budget)
        if k % 2:
            call = lambda: ctx.encode_images_budget_device([d.data_ptr() for d in d_frames], W, H, budget, index_interval=interval)
        else:
            call = lambda: ctx.encode_images_budget(frames, budget, index_interval=interval)
        if want is None:                                            # a quarter may lie below the smallest containers there are
            assert budget < smallest
            with pytest.raises(ia.MpcError) as e:
                call()
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT and str(budget) in str(e.value) and str(smallest) in str(e.value), str(e.value)
            continue
        got = call()
        j, probes = want
        info = got.info
        assert len(got) == n and got.size <= budget and probes <= 9
        assert (info.lambda_index, info.probes) == (j, probes), (budget, got)
        assert all((g.lambda_index, g.probes) == (j, probes) for g in got)
        _check_frames(ia, got, replay.at(j), frames, decode, interval)
        for field in ("full_bytes", "sse", "full_sse", "records", "full_records"):
            assert getattr(info, field) == sum(getattr(g, field) for g in got), field
        assert info.full_bytes == replay.full and [g.full_bytes for g in got] == [len(b) for b in fulls]
        assert [g.full_sse for g in got] == [_sse(rgb, decode(b)) for rgb, b in zip(frames, fulls)]
        assert [g.full_records for g in got] == [f.records for f in replay.frames]
        if budget == replay.full:
            assert j == -1 and [g.container for g in got] == fulls and all((g.depth == K).all() for g in got)
            assert info.sse == info.full_sse and info.records == info.full_records
        else:
            assert j >= 0 and info.records < info.full_records
            assert (replay.size(j - 1) if j > 0 else replay.full) > budget                        # the lo side is infeasible
        seen.add(j)
    assert -1 in seen and len(seen) >= 2, seen
    # one byte below the smallest containers there are: refused with both numbers
    for call in (lambda: ctx.encode_images_budget(frames, smallest - 1), lambda: ctx.encode_images_budget_device([d.data_ptr() for d in d_frames], W, H, smallest - 1)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and str(smallest - 1) in str(e.value) and str(smallest) in str(e.value), str(e.value)
    assert replay.search(smallest - 1) is None
    assert ctx.encode_images(frames) == fulls                       # the context is as it was


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("K", gc.KS)
@pytest.mark.parametrize("n", (1, 2, 3))
def test_group_quality_encode_end_to_end(ia, oracle, group_frames, n, K, fast):
    import torch
    ctx = _context(ia, K, fast)
    decode = _once(oracle.decode_image_fast if fast else oracle.decode_image)
    frames = group_frames[:n]
    fulls = ctx.encode_images(frames)
    replay = _replay(ia, ctx, group_frames, K, fast, n)
    D = replay.D
    assert all(a <= b for a, b in zip(D, D[1:])) and D[0] < D[255]
    d_frames = [torch.from_numpy(rgb).cuda() for rgb in frames]
    torch.cuda.synchronize()
    inner = sorted(set(D) - {D[0], D[255]})
    mid = inner[len(inner) // 2] if inner else D[255]
    seen = set()
    for k, target in enumerate((D[0], mid, mid - 1, D[255], (1 << 64) - 1)):
        interval = (None, 0, 32)[k % 3]
        if k % 2:
            got = ctx.encode_images_quality_device([d.data_ptr() for d in d_frames], W, H, max_sse=target, index_interval=interval)
        else:
            got = ctx.encode_images_quality(frames, max_sse=target, index_interval=interval)
        j = ia.quality_pick(replay.S, target)
        assert j >= 0 and j == max(i for i in range(gc.LAMBDAS) if D[i] <= target)
        info = got.info
        assert len(got) == n and info.lambda_index == j and all(g.lambda_index == j for g in got), (target, got)
        _check_frames(ia, got, replay.at(j), frames, decode, interval)
        assert info.sse == D[j] and info.sse <= target
        assert j == 255 or D[j + 1] > target
        assert info.records == int(replay.S[j, 2]) and info.model_bits_256 == int(replay.S[j, 1]) and info.min_sse == D[0]
        for field in ("full_bytes", "sse", "full_sse", "min_sse", "records", "full_records", "model_bits_256"):
            assert getattr(info, field) == sum(getattr(g, field) for g in got), field
        for f, g in enumerate(got):
            mine = replay.frames[f]
            assert g.min_sse == int(mine.S[0, 0]) and g.model_bits_256 == mine.at(j)[2][1] and g.full_bytes == len(fulls[f])
            assert g.full_sse == _sse(frames[f], decode(fulls[f])) and g.full_records == mine.records
        seen.add(j)
    assert 255 in seen and len(seen) >= 2, seen
    # one below the best that cutting reaches: refused with both figures
    if D[0] > 0:
        for call in (lambda: ctx.encode_images_quality(frames, max_sse=D[0] - 1), lambda: ctx.encode_images_quality_device([d.data_ptr() for d in d_frames], W, H, max_sse=D[0] - 1)):
            with pytest.raises(ia.MpcError) as e:
                call()
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT and str(D[0] - 1) in str(e.value) and str(D[0]) in str(e.value), str(e.value)
    # a PSNR target over the group's pixels
    psnr = 20.0 * math.log10(765.0) - 10.0 * math.log10(max(mid, 1) / (n * W * H)) - 0.01
    got = ctx.encode_images_quality(frames, psnr=psnr)
    assert got.info.lambda_index == ia.quality_pick(replay.S, ia.sse_for_psnr_group(psnr, W, H, n)) and got.info.sse <= ia.sse_for_psnr_group(psnr, W, H, n)
    assert ctx.encode_images(frames) == fulls


# ---- 4. one frame, the device forms, a neutral map --------------------------------------------------------------------------------

@pytest.mark.parametrize("fast", FLAVOURS)
def test_one_frame_is_the_single_frame_call(ia, group_frames, fast):
    K = 8
    ctx = _context(ia, K, fast)
    rgb = group_frames[0]
    rng = np.random.default_rng(3)
    full = ctx.encode_image(rgb)
    floor = _floor(ctx, [rgb])
    for emphasis in (None, rng.integers(0, 80, TILES).astype(np.uint8)):
        for budget in (len(full), floor + (len(full) - floor) // 2, floor + (len(full) - floor) // 5):
            for interval in (None, 0):
                one = ctx.encode_image_budget_emphasis(rgb, budget, emphasis, index_interval=interval)
                got = ctx.encode_images_budget([rgb], budget, emphasis=emphasis, index_interval=interval)
                assert len(got) == 1 and got[0].container == one.container and got[0].index == one.index and np.array_equal(got[0].depth, one.depth)
                assert repr(got[0]) == repr(one)
                assert all(getattr(got.info, f) == getattr(one, f) for f, _ in ia.api.MpcBudgetInfo._fields_)
        loose = ctx.encode_image_quality(rgb, max_sse=(1 << 63))
        for target in (loose.min_sse, 3 * loose.min_sse + 1000, loose.full_sse, 1 << 63):
            one = ctx.encode_image_quality_emphasis(rgb, emphasis, max_sse=target, index_interval=0)
            got = ctx.encode_images_quality([rgb], max_sse=target, emphasis=emphasis, index_interval=0)
            assert len(got) == 1 and got[0].container == one.container and got[0].index == one.index and np.array_equal(got[0].depth, one.depth)
            assert repr(got[0]) == repr(one)
            assert all(getattr(got.info, f) == getattr(one, f) for f, _ in ia.api.MpcQualityInfo._fields_)
    psnr = 20.0 * math.log10(765.0) - 10.0 * math.log10(3 * loose.min_sse / (W * H))        # a target that cutting reaches
    assert ia.sse_for_psnr_group(psnr, W, H, 1) == ia.sse_for_psnr(psnr, W, H) >= loose.min_sse
    assert repr(ctx.encode_images_quality([rgb], psnr=psnr)[0]) == repr(ctx.encode_image_quality(rgb, psnr=psnr))


@pytest.mark.parametrize("fast", FLAVOURS)
def test_device_forms_equal_host_forms_and_a_neutral_map_is_no_map(ia, group_frames, fast):
    import torch
    K = 8
    ctx = _context(ia, K, fast)
    frames = group_frames
    n = len(frames)
    fulls = ctx.encode_images(frames)
    total = sum(len(b) for b in fulls)
    d_frames = [torch.from_numpy(rgb).cuda() for rgb in frames]
    ptrs = [d.data_ptr() for d in d_frames]
    rng = np.random.default_rng(11)
    emphasis = rng.integers(1, 65, (n, TILES)).astype(np.uint8)
    neutral = np.full((n, TILES), 16, np.uint8)
    d_emphasis, d_neutral = torch.from_numpy(emphasis).cuda(), torch.from_numpy(neutral).cuda()
    torch.cuda.synchronize()

    def same(a, b):
        assert repr(a) == repr(b) and len(a) == len(b) == n
        for x, y in zip(a, b):
            assert repr(x) == repr(y) and x.container == y.container and x.index == y.index and np.array_equal(x.depth, y.depth)

    # the full containers fit: mpc_encode_images, byte for byte
    fits = ctx.encode_images_budget(frames, total, index_interval=0)
    assert [g.container for g in fits] == fulls and fits.info.lambda_index == -1 and fits.info.probes == 0 and fits.size == total
    plain = {}
    floor = _floor(ctx, frames)
    for budget in (total, floor + (total - floor) // 2, floor + (total - floor) // 4):
        plain[budget] = ctx.encode_images_budget(frames, budget, index_interval=0)
        same(plain[budget], ctx.encode_images_budget_device(ptrs, W, H, budget, index_interval=0))
        same(plain[budget], ctx.encode_images_budget(frames, budget, emphasis=neutral, index_interval=0))
        same(plain[budget], ctx.encode_images_budget_device(ptrs, W, H, budget, d_emphasis=d_neutral.data_ptr(), index_interval=0))
        assert plain[budget].size <= budget
        weighted = ctx.encode_images_budget(frames, budget, emphasis=emphasis, index_interval=0)
        same(weighted, ctx.encode_images_budget_device(ptrs, W, H, budget, d_emphasis=d_emphasis.data_ptr(), index_interval=0))
        assert weighted.size <= budget
    loose = ctx.encode_images_quality(frames, max_sse=(1 << 63))
    for target in (loose.info.min_sse, 2 * loose.info.min_sse + 5000, loose.info.full_sse):
        a = ctx.encode_images_quality(frames, max_sse=target, index_interval=0)
        same(a, ctx.encode_images_quality_device(ptrs, W, H, max_sse=target, index_interval=0))
        same(a, ctx.encode_images_quality(frames, max_sse=target, emphasis=neutral, index_interval=0))
        same(a, ctx.encode_images_quality_device(ptrs, W, H, max_sse=target, d_emphasis=d_neutral.data_ptr(), index_interval=0))
        b = ctx.encode_images_quality(frames, max_sse=target, emphasis=emphasis, index_interval=0)
        same(b, ctx.encode_images_quality_device(ptrs, W, H, max_sse=target, d_emphasis=d_emphasis.data_ptr(), index_interval=0))
        assert a.info.sse <= target and b.info.sse <= target
    assert ctx.encode_images(frames) == fulls


def test_a_group_beyond_one_chunk_of_frames(ia, oracle, group_frames):
    """nine frames: the kernels' second launch takes the ninth, whose result is its own whichever chunk it lies in"""
    K = 8
    ctx = _context(ia, K)
    frames = [group_frames[k % 4] if k < 4 else oracle.synth_frame(W, H, 100 + k) for k in range(9)]
    fulls = ctx.encode_images(frames)
    total = sum(len(b) for b in fulls)
    budget = (_floor(ctx, frames) + total) // 2
    got = ctx.encode_images_budget(frames, budget, index_interval=0)
    assert got.size <= budget and got.info.lambda_index >= 0
    j = got.info.lambda_index
    for f, rgb in enumerate(frames):
        blob, depth, totals = _Frame(ia, ctx, rgb).at(j)
        assert got[f].container == blob and np.array_equal(got[f].depth, depth) and got[f].sse == totals[0], f
        assert got[f].sse == _sse(rgb, oracle.decode_image(got[f].container)), f
    q = ctx.encode_images_quality(frames, max_sse=got.info.sse, index_interval=0)
    assert q.info.sse <= got.info.sse and q.info.lambda_index >= j
    assert ctx.encode_images(frames) == fulls


# ---- 5. refusals, and what the calls leave as they found it -----------------------------------------------------------------------

@pytest.mark.parametrize("fast", FLAVOURS)
def test_refusals_and_state(ia, group_frames, fast):
    import torch
    K = 8
    ctx = _context(ia, K, fast)
    frames = group_frames[:3]
    fulls = ctx.encode_images(frames)
    total = sum(len(b) for b in fulls)
    d_frames = [torch.from_numpy(rgb).cuda() for rgb in frames]
    ptrs = [d.data_ptr() for d in d_frames]
    d_counts = torch.zeros((TILES, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((TILES, 3, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_tiles_device(ptrs[0], W, H, 3 * W, 0, H // 8, d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    quant = ctx.quant
    half = (_floor(ctx, frames) + total) // 2
    good = ctx.encode_images_budget(frames, half)
    # a busy job slot: refused, and nothing of the call ran -- no pursuit was launched
    ctx.container_job_begin(3, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    for call in (lambda: ctx.encode_images_budget(frames, 1000), lambda: ctx.encode_images_budget_device(ptrs, W, H, 1000),
                 lambda: ctx.encode_images_quality(frames, max_sse=10 ** 9), lambda: ctx.encode_images_quality_device(ptrs, W, H, max_sse=10 ** 9)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "slot 3 is busy" in str(e.value)
    assert ctx.read_kernel_timing()[1] == 0
    ctx.container_job_cancel(3)
    assert [g.container for g in ctx.encode_images_budget(frames, half)] == [g.container for g in good]
    assert ctx.read_kernel_timing()[1] > 0
    ctx.kernel_timing(False)
    # the other refusals
    for bad in (lambda: ctx.encode_images_budget([], 1000), lambda: ctx.encode_images_budget([frames[0]] * 65, 1000),
                lambda: ctx.encode_images_quality([], max_sse=5), lambda: ctx.encode_images_quality_device([ptrs[0]] * 65, W, H, max_sse=5),
                lambda: ctx.encode_images_budget_device([ptrs[0], 0, ptrs[2]], W, H, 1000), lambda: ctx.encode_images_quality_device([0], W, H, max_sse=5),
                lambda: ctx.encode_images_budget(frames, 0), lambda: ctx.encode_images_budget(frames, 1000, index_interval=7),
                lambda: ctx.encode_images_quality(frames, max_sse=5, index_interval=1 << 20), lambda: ctx.encode_images_budget_device(ptrs, 0, H, 1000),
                lambda: ctx.encode_images_quality_device(ptrs, W, -1, max_sse=5), lambda: ctx.encode_images_quality(frames, psnr=float("nan"))):
        with pytest.raises(ia.MpcError) as e:
            bad()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    with pytest.raises(ValueError):
        ctx.encode_images_budget([frames[0], frames[1][:40]], 1000)
    host_only = ia.create_compression_context(K, 8, 3.5, device=-1)
    for call in (lambda: host_only.encode_images_budget(frames, 1000), lambda: host_only.encode_images_quality(frames, max_sse=10 ** 9)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host_only.close()
    # left as found: the quant tables, the fast flag -- also by a call with an override and by a refused one
    override = 2.0 * np.maximum(np.floor(quant), 1.0)
    with_override = ctx.encode_images_budget(frames, half, quant=override, index_interval=0)
    assert [g.container for g in with_override] != [g.container for g in good]
    assert np.array_equal(ctx.quant, quant) and ctx.fast == fast
    assert ctx.encode_images(frames) == fulls
    assert [g.container for g in ctx.encode_images_budget(frames, half)] == [g.container for g in good]
