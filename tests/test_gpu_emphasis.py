"""Emphasis maps on the device (run with -m gpu): each kernel against its host function on the cases of emphasis_cases.py, bit for bit;
the new _device entry points' stream contract through the harness of stream_order.py and their refusals with nothing enqueued; the
budget and the quality encode with a map end to end -- replayed with the public pieces alone, the reported error against the oracle's
decode, and a null or all-16 map against today's calls byte for byte; and the delta session with a map.  Every equality is exact."""
import numpy as np
import pytest

import delta_cases as dc
import emphasis_cases as ec
import quality_cases as qc
import rate_cases as rc
import stream_order as so

pytestmark = pytest.mark.gpu

CASES, FLOOR_CASES, MASK_CASES = ec.cases(large=True), ec.floor_cases(large=True), ec.mask_cases(wide=True)
POISON = 0x77


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


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(np.array(a.view(signed) if signed else a)).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _ints(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


# ---- 1. each kernel against its host function ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", ec.KS)
def test_allocation_and_sweep_kernels_are_the_host_functions(ia, K):
    import torch
    ctx = _context(ia, K)
    mine = [c for c in CASES if c[1].shape[1] == K + 1]
    assert {c[1].shape[0] for c in mine} >= set(ec.TILE_COUNTS) and any("wraps" in c[0] for c in mine)
    for name, P, counts, e, W, js, _ in mine:
        T = P.shape[0]
        d_profile, d_counts, d_e = _dev(P), _dev(counts), _dev(e)
        for j in js:
            d_depth = torch.full((T,), POISON, dtype=torch.uint8, device="cuda")
            d_cut = torch.full((T, 3), -1, dtype=torch.int16, device="cuda")
            d_totals = torch.full((3,), -1, dtype=torch.int64, device="cuda")
            ctx.budget_allocate_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e.data_ptr(), T, W, j, d_depth.data_ptr(), d_cut.data_ptr(),
                                                d_totals.data_ptr())
            torch.cuda.synchronize()
            depth, cut, totals = ia.budget_allocate_emphasis(P, counts, e, W, j)
            assert np.array_equal(_host(d_depth, np.uint8), depth) and np.array_equal(_host(d_cut, np.uint16), cut), (name, j)
            assert _ints(_host(d_totals, np.uint64)) == _ints(totals), (name, j)
        d_sweep = torch.full((ec.LAMBDAS, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        ctx.budget_sweep_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e.data_ptr(), T, W, d_sweep.data_ptr())
        torch.cuda.synchronize()
        want = ia.budget_sweep_emphasis(P, counts, e, W)
        got = _host(d_sweep, np.uint64)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        # a null map on the new entry points is the plain kernel
        ctx.budget_sweep_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), 0, T, W, d_sweep.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_host(d_sweep, np.uint64), ia.budget_sweep(P, counts, W)), name


@pytest.mark.parametrize("K", ec.KS)
def test_floor_allocation_kernel_is_the_host_function(ia, K):
    import torch
    ctx = _context(ia, K)
    mine = [c for c in FLOOR_CASES if c[1].shape[1] == K + 1]
    assert any(c[6] is None for c in mine) and any("outside" in c[0] for c in mine) and any(c[3] is None and c[4] is None for c in mine)
    for name, P, counts, floor, must, e, listed, W, js in mine:
        n = P.shape[0]
        d_profile, d_counts, d_e = _dev(P), _dev(counts), _dev(e)
        d_floor, d_must, d_list = (None if a is None else _dev(a) for a in (floor, must, listed))
        for j in js:
            d_depth = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
            d_send = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
            d_cut = torch.full((n, 3), -1, dtype=torch.int16, device="cuda")
            d_totals = torch.full((4,), -1, dtype=torch.int64, device="cuda")
            ctx.budget_allocate_floor_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), _ptr(d_floor), _ptr(d_must), d_e.data_ptr(), _ptr(d_list),
                                                      len(e), n, W, j, d_depth.data_ptr(), d_cut.data_ptr(), d_send.data_ptr(), d_totals.data_ptr())
            torch.cuda.synchronize()
            depth, cut, send, totals = ia.budget_allocate_floor_emphasis(P, counts, floor, must, e, listed, W, j)
            assert np.array_equal(_host(d_depth, np.uint8), depth) and np.array_equal(_host(d_send, np.uint8), send), (name, j)
            assert np.array_equal(_host(d_cut, np.uint16), cut) and _ints(_host(d_totals, np.uint64)) == _ints(totals), (name, j)


def _mask_device(torch, ctx, buffer, offset, width, height, lo, hi, stream=0):
    """-> the map, with the bytes around it: the output sits inside a poisoned buffer"""
    tiles = -(-width // 8) * -(-height // 8)
    d_mask = torch.from_numpy(buffer.reshape(-1).copy()).cuda()
    d_out = torch.full((tiles + 128,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.emphasis_from_mask_device(d_mask.data_ptr() + offset, width, height, d_out.data_ptr() + 61, lo, hi, row_stride=buffer.shape[1], stream=stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:61] == POISON).all() and (out[61 + tiles:] == POISON).all(), "a write outside the map"
    return out[61:61 + tiles]


def test_mask_kernel_is_the_host_function(ia):
    import torch
    ctx = _context(ia, 5)
    assert any(c[3] == 4928 for c in MASK_CASES)
    for name, buffer, offset, width, height, lo, hi in MASK_CASES:
        want = ia.emphasis_from_mask(ec.mask_view(buffer, offset, width, height), lo, hi)
        assert np.array_equal(_mask_device(torch, ctx, buffer, offset, width, height, lo, hi), want), name


# ---- 2. the stream contract -------------------------------------------------------------------------------------------------------

def _stream_inputs(K, T, seed):
    rng = np.random.default_rng(seed)
    _, P, counts, e, _, _, _ = ec._random_case(rng, K, T)
    return P, counts, e


def _entries(ia, ctx, K, T):
    """(name, inputs {name: (A, B)}, outputs {name: what A gives}, call(buffers)) of the four new _device entry points"""
    import budget_cases as bc
    (pa, ca, ea), (pb, cb, eb) = _stream_inputs(K, T, 41), _stream_inputs(K, T, 42)
    W = bc._weights(np.random.default_rng(43), K)
    j = 113
    depth, cut, totals = ia.budget_allocate_emphasis(pa, ca, ea, W, j)
    records = dict(profile=(pa, pb), counts=(ca, cb), emphasis=(ea, eb))

    def allocate(b):
        ctx.budget_allocate_emphasis_device(b.ptr("profile"), b.ptr("counts"), b.ptr("emphasis"), T, W, j, b.ptr("depth"), b.ptr("cut"), b.ptr("totals"),
                                            stream=b.stream)
        b.probe()

    def sweep(b):
        ctx.budget_sweep_emphasis_device(b.ptr("profile"), b.ptr("counts"), b.ptr("emphasis"), T, W, b.ptr("totals"), stream=b.stream)
        b.probe()

    rng = np.random.default_rng(44)
    floor, must = rng.integers(0, K + 1, T).astype(np.uint8), (rng.random(T) < 0.5).astype(np.uint8)
    la, lb = rng.permutation(T).astype(np.int32), rng.permutation(T).astype(np.int32)
    f_depth, f_cut, f_send, f_totals = ia.budget_allocate_floor_emphasis(pa, ca, floor, must, ea, la, W, j)

    def allocate_floor(b):
        ctx.budget_allocate_floor_emphasis_device(b.ptr("profile"), b.ptr("counts"), b.ptr("floor"), b.ptr("must"), b.ptr("emphasis"), b.ptr("list"), T, T,
                                                  W, j, b.ptr("depth"), b.ptr("cut"), b.ptr("send"), b.ptr("totals"), stream=b.stream)
        b.probe()

    width, height = 197, 117
    ma, mb = rng.integers(0, 256, (height, width)).astype(np.uint8), rng.integers(0, 256, (height, width)).astype(np.uint8)

    def mask(b):
        ctx.emphasis_from_mask_device(b.ptr("mask"), width, height, b.ptr("map"), 1, 64, stream=b.stream)
        b.probe()

    return [("budget_allocate_emphasis_device", records, dict(depth=depth, cut=cut, totals=totals), allocate),
            ("budget_sweep_emphasis_device", records, dict(totals=ia.budget_sweep_emphasis(pa, ca, ea, W)), sweep),
            ("budget_allocate_floor_emphasis_device", dict(records, floor=(floor, floor), must=(must, must), list=(la, lb)),
             dict(depth=f_depth, cut=f_cut, send=f_send, totals=f_totals), allocate_floor),
            ("emphasis_from_mask_device", dict(mask=(ma, mb)), dict(map=ia.emphasis_from_mask(ma, 1, 64)), mask)]


def test_the_device_entries_are_ordered_on_the_callers_stream_and_asynchronous(ia):
    import torch
    K, T = 5, 375
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    S = torch.cuda.Stream()
    cpm = so.cycles_per_ms(torch)
    try:
        for name, inputs, outputs, call in _entries(ia, ctx, K, T):
            _, _, warm = so.behind_delay(torch, S, call, inputs, outputs, 1000)
            delay = so.delay_ms_for(warm["host_ms"])
            got, _, info = so.behind_delay(torch, S, call, inputs, outputs, delay * cpm)
            print(f"{name}: warm-up enqueue {warm['host_ms']:.2f} ms, delay {delay:.0f} ms, enqueue behind the delay {info['host_ms']:.2f} ms, "
                  f"delay still running at return: {info['running']}")
            for key, want in outputs.items():
                assert np.array_equal(got[key], want), (name, key, int((got[key] != want).sum()))
            assert info["running"], f"{name} returned only after the stream had drained"
    finally:
        ctx.close()


def test_the_device_entries_refuse_a_capturing_stream_and_bad_arguments_with_nothing_enqueued(ia):
    import torch
    K, T = 5, 64
    fresh = ia.create_compression_context(K, 8, 3.5, device=0)
    try:
        S = torch.cuda.Stream()
        d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        marker = torch.zeros(16, dtype=torch.int32, device="cuda")
        W = np.full((3, K), 1000, np.uint32)
        p = d.data_ptr()
        calls = {"allocate": lambda s, **kw: fresh.budget_allocate_emphasis_device(kw.get("profile", p), p, p, kw.get("tiles", T), W, kw.get("j", 0), p, p,
                                                                                 kw.get("totals", p), stream=s),
                 "sweep": lambda s, **kw: fresh.budget_sweep_emphasis_device(kw.get("profile", p), p, p, kw.get("tiles", T), W, kw.get("totals", p), stream=s),
                 "floor": lambda s, **kw: fresh.budget_allocate_floor_emphasis_device(kw.get("profile", p), p, 0, 0, p, kw.get("list", p), kw.get("frame", T),
                                                                                    kw.get("tiles", T), W, kw.get("j", 0), p, p, p, kw.get("totals", p), stream=s),
                 "mask": lambda s, **kw: fresh.emphasis_from_mask_device(kw.get("profile", p), kw.get("width", 64), 64, kw.get("totals", p), kw.get("lo", 1),
                                                                       kw.get("hi", 64), row_stride=kw.get("stride", 0), stream=s)}
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=S):
            marker.add_(1)
            for name, call in calls.items():
                with pytest.raises(ia.MpcError) as e:
                    call(torch.cuda.current_stream().cuda_stream)
                assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "captured" in str(e.value), (name, str(e.value))
            marker.add_(1)
        torch.cuda.synchronize()
        assert int(marker[0]) == 0                                  # the capture ended cleanly and nothing ran
        graph.replay()
        torch.cuda.synchronize()
        assert int(marker[0]) == 2 and not d.cpu().numpy().any()    # the caller's two kernels and nothing else
        bad = [("allocate", dict(profile=0)), ("allocate", dict(totals=0)), ("allocate", dict(tiles=0)), ("allocate", dict(j=256)), ("allocate", dict(j=-1)),
               ("allocate", dict(tiles=(1 << 31) // 3 + 1)), ("sweep", dict(profile=0)), ("sweep", dict(totals=0)), ("sweep", dict(tiles=-5)),
               ("floor", dict(profile=0)), ("floor", dict(totals=0)), ("floor", dict(tiles=0)), ("floor", dict(j=256)), ("floor", dict(frame=0)),
               ("floor", dict(list=0, frame=T - 1)), ("mask", dict(profile=0)), ("mask", dict(totals=0)), ("mask", dict(width=0)), ("mask", dict(lo=0)),
               ("mask", dict(hi=65)), ("mask", dict(lo=9, hi=8)), ("mask", dict(stride=63))]
        for name, kw in bad:
            with pytest.raises(ia.MpcError) as e:
                calls[name](0, **kw)
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT, (name, kw)
        torch.cuda.synchronize()
        assert not d.cpu().numpy().any()
    finally:
        fresh.close()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------

def _sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


class _Replay:
    """the budget and the quality encode with a map from the public pieces alone: encode_tiles_device, the full container and its index,
    budget_weights, depth_profile_device, budget_sweep_emphasis_device, budget_allocate_emphasis_device, records_to_container_device"""

    def __init__(self, ia, ctx, rgb, emphasis):
        import torch
        self.ia, self.ctx, self.torch = ia, ctx, torch
        self.H, self.W = rgb.shape[:2]
        self.K, self.tiles = ctx.K, -(-self.W // 8) * -(-self.H // 8)
        self.d_rgb = torch.from_numpy(rgb).cuda()
        self.d_e = None if emphasis is None else torch.from_numpy(np.ascontiguousarray(emphasis)).cuda()
        self.d_counts = torch.zeros((self.tiles, 3), dtype=torch.int16, device="cuda")
        self.d_choices = torch.zeros((self.tiles, 3, self.K), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.encode_tiles_device(self.d_rgb.data_ptr(), self.W, self.H, 3 * self.W, 0, -(-self.H // 8), self.d_counts.data_ptr(), self.d_choices.data_ptr())
        torch.cuda.synchronize()
        self.full = bytes(ctx.records_to_container_device(self.d_counts.data_ptr(), self.d_choices.data_ptr(), self.W, self.H))
        self.weights = ia.budget_weights(ia.container_index(self.full))
        self.d_profile = torch.full((self.tiles, self.K + 1), -1, dtype=torch.int32, device="cuda")
        ctx.depth_profile_device(self.d_counts.data_ptr(), self.d_choices.data_ptr(), self.d_rgb.data_ptr(), self.W, self.H, self.d_profile.data_ptr())
        d_totals = torch.full((ec.LAMBDAS, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.budget_sweep_emphasis_device(self.d_profile.data_ptr(), self.d_counts.data_ptr(), _ptr(self.d_e), self.tiles, self.weights, d_totals.data_ptr())
        torch.cuda.synchronize()
        self.S = d_totals.cpu().numpy().view(np.uint64)
        self.made = {}

    def at(self, j):
        """-> (container, depth, totals) of the allocation at multiplier j"""
        if j not in self.made:
            torch = self.torch
            d_depth = torch.full((self.tiles,), POISON, dtype=torch.uint8, device="cuda")
            d_cut = torch.full((self.tiles, 3), -1, dtype=torch.int16, device="cuda")
            d_totals = torch.full((3,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            self.ctx.budget_allocate_emphasis_device(self.d_profile.data_ptr(), self.d_counts.data_ptr(), _ptr(self.d_e), self.tiles, self.weights, j,
                                                     d_depth.data_ptr(), d_cut.data_ptr(), d_totals.data_ptr())
            torch.cuda.synchronize()
            blob = bytes(self.ctx.records_to_container_device(d_cut.data_ptr(), self.d_choices.data_ptr(), self.W, self.H))
            self.made[j] = (blob, d_depth.cpu().numpy(), _ints(d_totals.cpu().numpy().view(np.uint64)))
        return self.made[j]

    def budget(self, budget):
        """mpc_encode_image_budget's search -> (lambda_index, probes, container, depth, totals)"""
        if len(self.full) <= budget:
            return -1, 0, self.full, np.full(self.tiles, self.K, np.uint8), None
        probed = {255}
        assert len(self.at(255)[0]) <= budget
        lo, hi = -1, 255
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            probed.add(mid)
            if len(self.at(mid)[0]) <= budget:
                hi = mid
            else:
                lo = mid
        return (hi, len(probed)) + self.at(hi)


def _same_result(a, b):
    return repr(a) == repr(b) and a.container == b.container and a.index == b.index and np.array_equal(a.depth, b.depth)


@pytest.mark.parametrize("fast", (False, True))
@pytest.mark.parametrize("K", qc.FRAME_KS)
@pytest.mark.parametrize("frame", qc.FRAMES, ids=[f[0] for f in qc.FRAMES])
def test_budget_and_quality_encode_with_a_map_end_to_end(ia, oracle, frame, K, fast):
    import torch
    name, W, H, seed = frame
    ctx = _context(ia, K, fast)
    decode = oracle.decode_image_fast if fast else oracle.decode_image
    rgb = oracle.synth_frame(W, H, seed)
    e = ec.central_map(W, H, 64, 4)
    assert 0 < int((e == 64).sum()) < e.size
    replay = _Replay(ia, ctx, rgb, e)
    full = ctx.encode_image(rgb)
    assert replay.full == full
    d_rgb, d_e = replay.d_rgb, replay.d_e
    host_S = ia.budget_sweep_emphasis(_host(replay.d_profile, np.uint32), _host(replay.d_counts, np.uint16), e, replay.weights)
    assert np.array_equal(replay.S, host_S)
    D = _ints(replay.S[:, 0])
    assert all(a <= b for a, b in zip(D, D[1:])) and D[0] < D[255]
    # the budget call
    cut_somewhere = False
    for k, quarters in enumerate((5, 3, 2)):
        budget = len(full) * quarters // 4
        interval = (None, 0, 32)[k % 3]
        want = replay.budget(budget)                                 # the smallest container is today's: at j = 255 no map keeps a record
        got = (ctx.encode_image_budget_emphasis_device(d_rgb.data_ptr(), W, H, budget, d_e.data_ptr(), index_interval=interval) if k % 2 else
               ctx.encode_image_budget_emphasis(rgb, budget, e, index_interval=interval))
        assert (got.lambda_index, got.probes) == want[:2] and got.container == want[2] and np.array_equal(got.depth, want[3]), (quarters, got)
        assert len(got.container) <= budget
        assert got.sse == _sse(rgb, decode(got.container)), (quarters, got)
        if want[4] is not None:
            assert got.sse == want[4][0] and got.records == want[4][2]
            cut_somewhere = True
        if interval is not None:
            assert got.index == ia.container_index2(got.container, interval, ia.api.MPC_INDEX_EXPANDED)
        assert got.full_bytes == len(full)
    assert cut_somewhere
    a = ctx.encode_image_budget_emphasis(rgb, len(full) // 2, e, index_interval=0)
    b = ctx.encode_image_budget_emphasis_device(d_rgb.data_ptr(), W, H, len(full) // 2, d_e.data_ptr(), index_interval=0)
    assert _same_result(a, b)
    # the quality call
    inner = sorted(set(D) - {D[0], D[255]})
    mid = inner[len(inner) // 2]
    for k, target in enumerate((D[0], mid, mid - 1, D[255])):
        got = (ctx.encode_image_quality_emphasis_device(d_rgb.data_ptr(), W, H, d_e.data_ptr(), max_sse=target, index_interval=0) if k % 2 else
               ctx.encode_image_quality_emphasis(rgb, e, max_sse=target, index_interval=0))
        j = ia.quality_pick(replay.S, target)
        assert j == max(i for i in range(ec.LAMBDAS) if D[i] <= target) and (j == 255 or D[j + 1] > target)
        blob, depth, totals = replay.at(j)
        assert got.lambda_index == j and got.container == blob and np.array_equal(got.depth, depth), (target, got)
        assert got.sse <= target and got.sse == D[j] == totals[0] == _sse(rgb, decode(got.container)), (target, got)
        assert got.records == totals[2] and got.model_bits_256 == totals[1] and got.min_sse == D[0]
        assert got.index == ia.container_index2(got.container, 0, ia.api.MPC_INDEX_EXPANDED)
    with pytest.raises(ia.MpcError) as err:
        ctx.encode_image_quality_emphasis(rgb, e, max_sse=D[0] - 1)
    assert err.value.status == ia.api.MPC_ERR_ARGUMENT and str(D[0]) in str(err.value)
    # the map moves error out of the centre: at one multiplier the emphasised tiles are no worse and the others no better than without it
    plain = _Replay(ia, ctx, rgb, None)
    j = ia.quality_pick(replay.S, mid)
    P = _host(replay.d_profile, np.uint32)
    rows = np.arange(P.shape[0])
    with_map, without = P[rows, replay.at(j)[1]].astype(np.int64), P[rows, plain.at(j)[1]].astype(np.int64)
    assert (with_map[e == 64] <= without[e == 64]).all() and (with_map[e == 4] >= without[e == 4]).all() and (with_map != without).any()
    # no map and the neutral map: today's calls, byte for byte
    d_16 = torch.full((e.size,), 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    budget = len(full) // 2
    today = ctx.encode_image_budget(rgb, budget, index_interval=0)
    assert _same_result(ctx.encode_image_budget_device(d_rgb.data_ptr(), W, H, budget, index_interval=0), today)
    for got in (ctx.encode_image_budget_emphasis(rgb, budget, None, index_interval=0), ctx.encode_image_budget_emphasis(rgb, budget, np.full(e.size, 16, np.uint8), index_interval=0),
                ctx.encode_image_budget_emphasis_device(d_rgb.data_ptr(), W, H, budget, 0, index_interval=0),
                ctx.encode_image_budget_emphasis_device(d_rgb.data_ptr(), W, H, budget, d_16.data_ptr(), index_interval=0)):
        assert _same_result(got, today)
    assert not _same_result(a, today)
    today = ctx.encode_image_quality(rgb, max_sse=mid, index_interval=0)
    assert _same_result(ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=mid, index_interval=0), today)
    for got in (ctx.encode_image_quality_emphasis(rgb, None, max_sse=mid, index_interval=0),
                ctx.encode_image_quality_emphasis(rgb, np.full(e.size, 16, np.uint8), max_sse=mid, index_interval=0),
                ctx.encode_image_quality_emphasis_device(d_rgb.data_ptr(), W, H, 0, max_sse=mid, index_interval=0),
                ctx.encode_image_quality_emphasis_device(d_rgb.data_ptr(), W, H, d_16.data_ptr(), max_sse=mid, index_interval=0)):
        assert _same_result(got, today)
    assert ctx.encode_image(rgb) == full                             # the context is as it was


def test_encode_refusals_leave_nothing_enqueued_and_the_slots_usable(ia, oracle):
    import torch
    K = 8
    _, W, H, seed = qc.FRAMES[0]
    ctx = _context(ia, K)
    rgb = oracle.synth_frame(W, H, seed)
    e = ec.central_map(W, H)
    d_rgb, d_e = torch.from_numpy(rgb).cuda(), torch.from_numpy(e).cuda()
    tiles = e.size
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, -(-H // 8), d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    full = ctx.encode_image(rgb)
    good = ctx.encode_image_budget_emphasis(rgb, len(full) // 2, e)
    calls = (lambda **kw: ctx.encode_image_budget_emphasis(rgb, kw.get("budget", len(full) // 2), e, index_interval=kw.get("interval")),
             lambda **kw: ctx.encode_image_budget_emphasis_device(kw.get("px", d_rgb.data_ptr()), kw.get("W", W), H, kw.get("budget", len(full) // 2), d_e.data_ptr(),
                                                                  index_interval=kw.get("interval")),
             lambda **kw: ctx.encode_image_quality_emphasis(rgb, e, max_sse=10 ** 9, index_interval=kw.get("interval")),
             lambda **kw: ctx.encode_image_quality_emphasis_device(kw.get("px", d_rgb.data_ptr()), kw.get("W", W), H, d_e.data_ptr(), max_sse=10 ** 9,
                                                                   index_interval=kw.get("interval")))
    # a busy job slot: refused, and nothing of the call ran -- no pursuit was launched; the slot left idle is usable after each refusal
    ctx.container_job_begin(3, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    for call in calls:
        with pytest.raises(ia.MpcError) as err:
            call()
        assert err.value.status == ia.api.MPC_ERR_ARGUMENT and "slot 3 is busy" in str(err.value)
        assert bytes(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), W, H)) == full       # slot 0 was left idle
    assert ctx.read_kernel_timing()[1] == 0
    ctx.container_job_cancel(3)
    ctx.kernel_timing(False)
    for call in calls:
        for kw in (dict(interval=7), dict(interval=1 << 20)) + ((dict(px=0), dict(W=0)) if call in (calls[1], calls[3]) else ()):
            with pytest.raises(ia.MpcError) as err:
                call(**kw)
            assert err.value.status == ia.api.MPC_ERR_ARGUMENT, kw
    for call in calls[:2]:
        with pytest.raises(ia.MpcError) as err:
            call(budget=0)
        assert err.value.status == ia.api.MPC_ERR_ARGUMENT
    with pytest.raises(ValueError):
        ctx.encode_image_budget_emphasis(rgb, len(full), e[:-1])
    assert ctx.encode_image_budget_emphasis(rgb, len(full) // 2, e).container == good.container and ctx.encode_image(rgb) == full


# ---- 4. the session ---------------------------------------------------------------------------------------------------------------

def _session_pieces(ia, ctx, name):
    from test_gpu_rate import DevicePieces
    return DevicePieces(ia, ctx, name)


@pytest.mark.parametrize("fast", (False, True))
def test_a_key_budget_call_with_a_map_is_the_single_frame_encode_with_that_map(ia, fast):
    name = "ragged"
    w, h, K = dc.SHAPES[name]
    ctx = ia.create_compression_context(K, 8, dc.QUALITY, device=0).set_fast(fast)
    try:
        px = np.array(dc.frame(w, h, 21))
        e = ec.central_map(w, h)
        d_px, d_e = _dev(px), _dev(e)
        full = ctx.encode_image(px, quant=dc.quant(name))
        enc = ctx.delta_encoder(w, h)
        enc.set_emphasis(e)
        differs = False
        for budget in (len(full) + 40, len(full) // 2 + 40, len(full) // 3 + 40):
            patch, info = enc.encode_patch_budget(px, budget, quant=dc.quant(name), key=True)
            want = ctx.encode_image_budget_emphasis_device(d_px.data_ptr(), w, h, budget - 40, d_e.data_ptr(), quant=dc.quant(name))
            pinfo = ia.patch_info(patch)
            assert pinfo["key"] == 1 and len(patch) <= budget and patch[pinfo["container_offset"]:] == want.container, budget
            assert (info.lambda_index, info.probes, info.sse) == (want.lambda_index, want.probes, want.sse), budget
            assert np.array_equal(enc.sent(), want.depth)
            differs = differs or want.container != ctx.encode_image_budget_device(d_px.data_ptr(), w, h, budget - 40, quant=dc.quant(name)).container
        assert differs
        enc.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("fast", (False, True))
def test_a_tight_stream_with_a_map(ia, fast):
    """three frames under a budget of a third of the key frame's patch: every patch is the replay's (rate_cases.Replay with the floor
    allocation of emphasis_cases), and a twin receiver holds exactly the decode of the records cut to the sent map after every call;
    set_emphasis(None) restores today's patches; a map of the wrong size is refused and the session stays usable"""
    name = "ragged"
    w, h, K = dc.SHAPES[name]
    ctx = ia.create_compression_context(K, 8, dc.QUALITY, device=0).set_fast(fast)
    try:
        pieces = _session_pieces(ia, ctx, name)
        frames = rc.base_sequence(name)[:3]
        e = ec.central_map(w, h)
        T = e.size
        loose = rc.Replay(pieces, w, h, K).call(frames[0], 1 << 40)
        budget = loose["all_bytes"] // 3
        with_map, without = ec.Replay(pieces, w, h, K), rc.Replay(pieces, w, h, K)
        with_map.emphasis = e
        enc, plain, dec = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h), ctx.patch_decoder(w, h)
        with pytest.raises(ia.MpcError) as err:
            enc.set_emphasis(e[:-1])
        assert err.value.status == ia.api.MPC_ERR_ARGUMENT
        enc.set_emphasis(e)
        header_quant, cut, moved = None, False, False
        for i, px in enumerate(frames):
            r, r0 = with_map.call(px, budget), without.call(px, budget)
            assert r is not None and r0 is not None, "the budget is below a call's smallest patch"
            patch, info = enc.encode_patch_budget(px, budget, quant=dc.quant(name))
            assert len(patch) <= budget and patch == r["patch"], (i, info)
            sent = enc.sent()
            assert np.array_equal(sent, r["sent"]), i
            for field in ("changed", "candidates", "sent_tiles", "owed", "lambda_index", "probes", "all_bytes", "key"):
                assert getattr(info, field) == r[field], (i, field, info)
            cut = cut or r["lambda_index"] >= 0
            moved = moved or r["patch"] != r0["patch"]
            dec.apply(patch)
            if header_quant is None:
                header_quant = ia.read_compressed(patch[ia.patch_info(patch)["container_offset"]:])["quant"]
            assert np.array_equal(dec.frame(), pieces.decode_cut(px, sent, header_quant)), i                    # THE INVARIANT
            if i == 1:                                               # a refusal in the middle: the session goes on as if nothing had happened
                with pytest.raises(ia.MpcError):
                    enc.set_emphasis(np.full(T + 1, 16, np.uint8))
            # the twin without a map, and one whose map was set and taken back: today's patches
            plain.set_emphasis(e)
            plain.set_emphasis(None)
            assert plain.encode_patch_budget(px, budget, quant=dc.quant(name))[0] == r0["patch"], i
        assert cut and moved
        # encode_patch ignores the map
        mapped, other = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
        mapped.set_emphasis(e)
        for px in frames:
            assert mapped.encode_patch(px, quant=dc.quant(name)) == other.encode_patch(px, quant=dc.quant(name))
        for s in (enc, plain, dec, mapped, other):
            s.close()
    finally:
        ctx.close()
