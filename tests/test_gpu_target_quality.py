"""Encode to a target quality on the device (run with -m gpu): the sweep kernel against mpc_budget_sweep on the cases of
quality_cases.py, all 768 words; mpc_budget_sweep_device's stream contract through the harness of stream_order.py and its refusal of a
capturing stream; mpc_encode_image_quality[_device] end to end -- the call replayed with the public pieces alone, the reported error
against the oracle's decode, the pick against the frame's own sweep, refusals and what the call leaves as it found it; and
mpc_encode_image_budget against the bytes it returned at the commit in front of this feature (tests/golden/budget_bytes_parent.json),
and the quality encode, the encodes with an emphasis map and the delta stream to a budget against theirs at the commit in front of
their shared front end (tests/golden/cut_bytes_parent.json).  Every equality is exact.

The file's name sorts it behind test_gpu_stream_order.py on purpose.  That module's control
(test_control_the_null_stream_does_not_see_a) needs the null stream's work to run while a side stream is held back, which depends on
which hardware queue the side stream gets; as test_gpu_quality.py this file ran first, its five torch streams and six contexts moved
that assignment, and the control -- code this feature does not touch -- saw A's records (observed once on an MI355X, in a whole
`-m gpu` run; behind the stream modules the suite is green)."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import budget_cases as bc
import quality_cases as qc
import stream_order as so
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FLAVOURS = (False, True)


def _device_constant(name):
    with open(os.path.join(ROOT, "imageexperiments_amd", "csrc", "mp_device.h")) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


GRID_CAP, CHUNK = _device_constant("kSweepGridCap"), _device_constant("kSweepTiles")


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


# ---- 1. the sweep kernel ----------------------------------------------------------------------------------------------------------

def _wrap_cases():
    """more tiles than the grid cap, and more chunks than the grid cap: there the grid-stride loop goes round four times"""
    rng = np.random.default_rng(99)
    out = []
    for K, T in ((8, 4 * GRID_CAP + 3), (1, 4 * GRID_CAP * CHUNK + 3)):
        counts = rng.integers(0, K + 2, (T, 3)).astype(np.uint16)
        P = bc._consistent_profile(rng, np.minimum(counts, K), K, monotone=False)
        out.append((f"K{K} T{T} wraps", P, counts, bc._weights(rng, K)))
    return out


SWEEP_CASES = qc.cases() + _wrap_cases()


def _sweep_device(torch, ctx, d_profile, d_counts, tiles, W, stream):
    d_totals = torch.full((qc.LAMBDAS, 3), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")       # garbage: the call zeroes it
    torch.cuda.synchronize()
    ctx.budget_sweep_device(d_profile.data_ptr(), d_counts.data_ptr(), tiles, W, d_totals.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    return d_totals.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("K", (1, 8, 32))
def test_sweep_kernel_is_the_host_function(ia, K):
    import torch
    ctx = _context(ia, K)
    S = torch.cuda.Stream()
    mine = [c for c in SWEEP_CASES if c[1].shape[1] == K + 1]
    assert len(mine) >= 8
    for name, P, counts, W in mine:
        d_profile = torch.from_numpy(P.view(np.int32).copy()).cuda()
        d_counts = torch.from_numpy(counts.view(np.int16).copy()).cuda()
        want = ia.budget_sweep(P, counts, W)
        got = _sweep_device(torch, ctx, d_profile, d_counts, P.shape[0], W, S)
        assert got.shape == (qc.LAMBDAS, 3) and np.array_equal(got, want), (name, int((got != want).sum()))
        again = _sweep_device(torch, ctx, d_profile, d_counts, P.shape[0], W, S)
        assert np.array_equal(again, got), name
    assert any("wraps" in c[0] for c in mine) or K == 32


# ---- 2. the stream contract -------------------------------------------------------------------------------------------------------

def test_sweep_device_is_ordered_on_the_callers_stream_and_asynchronous(ia):
    import torch
    K, T = 8, 375
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)

    def inputs(seed):
        rng = np.random.default_rng(seed)
        counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
        return bc._consistent_profile(rng, counts, K, monotone=False), counts

    (pa, ca), (pb, cb) = inputs(31), inputs(32)
    weights = bc._weights(np.random.default_rng(33), K)
    want, other = ia.budget_sweep(pa, ca, weights), ia.budget_sweep(pb, cb, weights)
    assert not np.array_equal(want, other)

    def call(b):
        ctx.budget_sweep_device(b.ptr("profile"), b.ptr("counts"), T, weights, b.ptr("totals"), stream=b.stream)
        b.probe()

    S = torch.cuda.Stream()
    cpm = so.cycles_per_ms(torch)
    try:
        io = dict(inputs={"profile": (pa, pb), "counts": (ca, cb)}, outputs={"totals": want})
        _, _, warm = so.behind_delay(torch, S, call, io["inputs"], io["outputs"], 1000)
        delay = so.delay_ms_for(warm["host_ms"])
        got, _, info = so.behind_delay(torch, S, call, io["inputs"], io["outputs"], delay * cpm)
        print(f"budget_sweep_device: warm-up enqueue {warm['host_ms']:.2f} ms, delay {delay:.0f} ms, enqueue behind the delay "
              f"{info['host_ms']:.2f} ms, delay still running at return: {info['running']}")
        assert np.array_equal(got["totals"], want), int((got["totals"] != want).sum())
        assert info["running"], "budget_sweep_device returned only after the stream had drained"
    finally:
        ctx.close()


def test_sweep_device_refuses_a_capturing_stream_on_a_context_that_has_made_no_call(ia):
    import torch
    K, T = 8, 375
    fresh = ia.create_compression_context(K, 8, 3.5, device=0)
    try:
        S = torch.cuda.Stream()
        d = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
        marker = torch.zeros(16, dtype=torch.int32, device="cuda")
        weights = np.full((3, K), 1000, np.uint32)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=S):
            marker.add_(1)
            with pytest.raises(ia.MpcError) as e:
                fresh.budget_sweep_device(d.data_ptr(), d.data_ptr(), T, weights, d.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "captured" in str(e.value), str(e.value)
            marker.add_(1)
        torch.cuda.synchronize()
        assert int(marker[0]) == 0                                  # the capture ended cleanly and nothing ran
        graph.replay()
        torch.cuda.synchronize()
        assert int(marker[0]) == 2 and not d.cpu().numpy().any()    # the caller's two kernels and nothing else
        # the other refusals: nothing enqueued either
        for args in ((0, d.data_ptr(), T, d.data_ptr()), (d.data_ptr(), 0, T, d.data_ptr()), (d.data_ptr(), d.data_ptr(), T, 0),
                     (d.data_ptr(), d.data_ptr(), 0, d.data_ptr()), (d.data_ptr(), d.data_ptr(), -5, d.data_ptr()),
                     (d.data_ptr(), d.data_ptr(), (1 << 31) // 3 + 1, d.data_ptr())):
            with pytest.raises(ia.MpcError) as e:
                fresh.budget_sweep_device(args[0] or None, args[1] or None, args[2], weights, args[3] or None)
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT
        torch.cuda.synchronize()
        assert not d.cpu().numpy().any()
        host_only = ia.create_compression_context(K, 8, 3.5, device=-1)
        with pytest.raises(ia.MpcError) as e:
            host_only.budget_sweep_device(d.data_ptr(), d.data_ptr(), T, weights, d.data_ptr())
        assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
        host_only.close()
    finally:
        fresh.close()


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------

def _sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


class _Replay:
    """mpc_encode_image_quality with the public pieces alone: encode_tiles_device, container and index, budget_weights,
    depth_profile_device, budget_sweep_device, quality_pick, budget_allocate_device, records_to_container_device"""

    def __init__(self, ia, ctx, rgb):
        import torch
        self.ia, self.ctx, self.torch = ia, ctx, torch
        self.H, self.W = rgb.shape[:2]
        self.K, self.tiles = ctx.K, -(-self.W // 8) * -(-self.H // 8)
        self.d_rgb = torch.from_numpy(rgb).cuda()
        self.d_counts = torch.zeros((self.tiles, 3), dtype=torch.int16, device="cuda")
        self.d_choices = torch.zeros((self.tiles, 3, self.K), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.encode_tiles_device(self.d_rgb.data_ptr(), self.W, self.H, 3 * self.W, 0, -(-self.H // 8), self.d_counts.data_ptr(),
                                self.d_choices.data_ptr())
        torch.cuda.synchronize()
        self.full = bytes(ctx.records_to_container_device(self.d_counts.data_ptr(), self.d_choices.data_ptr(), self.W, self.H))
        self.weights = ia.budget_weights(ia.container_index(self.full))
        self.d_profile = torch.full((self.tiles, self.K + 1), -1, dtype=torch.int32, device="cuda")
        ctx.depth_profile_device(self.d_counts.data_ptr(), self.d_choices.data_ptr(), self.d_rgb.data_ptr(), self.W, self.H, self.d_profile.data_ptr())
        d_totals = torch.full((qc.LAMBDAS, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.budget_sweep_device(self.d_profile.data_ptr(), self.d_counts.data_ptr(), self.tiles, self.weights, d_totals.data_ptr())
        torch.cuda.synchronize()
        self.S = d_totals.cpu().numpy().view(np.uint64)
        self.D = [int(v) for v in self.S[:, 0]]
        self.made = {}

    def at(self, j):
        """-> (container, depth, totals) of the allocation at multiplier j"""
        if j not in self.made:
            torch = self.torch
            d_depth = torch.full((self.tiles,), -1, dtype=torch.uint8, device="cuda")
            d_cut = torch.full((self.tiles, 3), -1, dtype=torch.int16, device="cuda")
            d_totals = torch.full((3,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            self.ctx.budget_allocate_device(self.d_profile.data_ptr(), self.d_counts.data_ptr(), self.tiles, self.weights, j, d_depth.data_ptr(),
                                            d_cut.data_ptr(), d_totals.data_ptr())
            torch.cuda.synchronize()
            blob = bytes(self.ctx.records_to_container_device(d_cut.data_ptr(), self.d_choices.data_ptr(), self.W, self.H))
            self.made[j] = (blob, d_depth.cpu().numpy(), [int(v) for v in d_totals.cpu().numpy().view(np.uint64)])
        return self.made[j]


@pytest.mark.parametrize("fast", FLAVOURS)
@pytest.mark.parametrize("K", qc.FRAME_KS)
@pytest.mark.parametrize("frame", qc.FRAMES, ids=[f[0] for f in qc.FRAMES])
def test_quality_encode_end_to_end(ia, oracle, frame, K, fast):
    name, W, H, seed = frame
    ctx = _context(ia, K, fast)
    decode = oracle.decode_image_fast if fast else oracle.decode_image
    rgb = oracle.synth_frame(W, H, seed)
    full = ctx.encode_image(rgb)
    replay = _Replay(ia, ctx, rgb)
    D = replay.D
    assert replay.full == full and np.array_equal(replay.S, ia.budget_sweep(replay.d_profile.cpu().numpy().view(np.uint32), replay.d_counts.cpu().numpy().view(np.uint16), replay.weights))
    assert all(a <= b for a, b in zip(D, D[1:])) and D[0] > 0 and D[0] < D[255]
    full_sse = _sse(rgb, decode(full))
    assert D[0] <= full_sse
    inner = sorted(set(D) - {D[0], D[255]})
    mid = inner[len(inner) // 2]
    d_rgb = replay.d_rgb
    seen = set()
    for k, target in enumerate((D[0], mid, mid - 1, D[255], qc.U64_MAX, full_sse)):
        interval = (None, 0, 32)[k % 3]
        if k % 2:
            got = ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=target, index_interval=interval)
        else:
            got = ctx.encode_image_quality(rgb, max_sse=target, index_interval=interval)
        j = ia.quality_pick(replay.S, target)
        assert j >= 0 and j == max(i for i in range(qc.LAMBDAS) if D[i] <= target)
        blob, depth, totals = replay.at(j)
        assert got.lambda_index == j and got.container == blob, (target, got)                      # (a)
        assert got.sse == _sse(rgb, decode(got.container)) and got.sse <= target, (target, got)    # (b)
        assert got.sse == D[j] == totals[0]
        assert j == 255 or D[j + 1] > target                                                       # (c)
        assert np.array_equal(got.depth, depth)                                                    # (d)
        if interval is None:
            assert got.index is None
        else:
            assert got.index == ia.container_index2(got.container, interval, ia.api.MPC_INDEX_EXPANDED), target     # (e)
        assert got.full_bytes == len(full) and got.full_sse == full_sse and got.min_sse == D[0]
        assert got.records == totals[2] == int(replay.S[j, 2]) and got.model_bits_256 == totals[1] == int(replay.S[j, 1])
        assert got.full_records == int(np.minimum(replay.d_counts.cpu().numpy().view(np.uint16), K).sum()) and got.records <= got.full_records
        seen.add(j)
        assert ctx.encode_image(rgb) == full                                                       # the context is as it was
    assert {255} <= seen and len(seen) >= 4, seen
    # a target looser than the full container's own error still cuts: fewer records, fewer bytes
    loose = ctx.encode_image_quality(rgb, max_sse=D[255])
    assert loose.records == 0 and len(loose.container) < len(full) and not loose.depth.any()
    # host and device pixels: one result
    a, b = ctx.encode_image_quality(rgb, max_sse=mid, index_interval=0), ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=mid, index_interval=0)
    assert repr(a) == repr(b) and a.container == b.container and a.index == b.index and np.array_equal(a.depth, b.depth)
    # one below the best that cutting reaches: refused with both figures, and the context usable
    for call in (lambda: ctx.encode_image_quality(rgb, max_sse=D[0] - 1), lambda: ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=D[0] - 1)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and str(D[0] - 1) in str(e.value) and str(D[0]) in str(e.value), str(e.value)
    assert ia.quality_pick(replay.S, D[0] - 1) == -1
    assert ctx.encode_image(rgb) == full and ctx.encode_image_quality(rgb, max_sse=D[0]).container == replay.at(ia.quality_pick(replay.S, D[0]))[0]
    # (f) a PSNR target: two dB below the full container's
    target = ia.calculate_psnr(rgb, decode(full)) - 2.0
    got = ctx.encode_image_quality(rgb, psnr=target)
    assert ia.calculate_psnr(rgb, decode(got.container)) >= target
    assert got.sse <= ia.sse_for_psnr(target, W, H) and got.lambda_index == ia.quality_pick(replay.S, ia.sse_for_psnr(target, W, H))
    assert got.lambda_index > 0 and len(got.container) < len(full)


# ---- 4. refusals, and what the call leaves as it found it -------------------------------------------------------------------------

@pytest.mark.parametrize("fast", FLAVOURS)
def test_refusals_and_state(ia, oracle, fast):
    import torch
    K = 8
    _, W, H, seed = qc.FRAMES[0]
    ctx = _context(ia, K, fast)
    rgb = oracle.synth_frame(W, H, seed)
    full = ctx.encode_image(rgb)
    d_rgb = torch.from_numpy(rgb).cuda()
    tiles = -(-W // 8) * -(-H // 8)
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, -(-H // 8), d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    workgroups = ctx.L.mpc_context_tile_encode_workgroups
    workgroups.argtypes, workgroups.restype = [ia.api.C.c_void_p], ia.api.C.c_int
    ctx.set_tile_encode_workgroups(100)
    quant = ctx.quant
    good =ctx.encode_image_quality(rgb, max_sse=qc.U64_MAX // 2)
    # a busy job slot: refused, and nothing of the call ran -- no pursuit was launched
    ctx.container_job_begin(3, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    for call in (lambda: ctx.encode_image_quality(rgb, max_sse=10 ** 9), lambda: ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=10 ** 9)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT and "slot 3 is busy" in str(e.value)
    assert ctx.read_kernel_timing()[1] == 0
    ctx.container_job_cancel(3)
    assert ctx.encode_image_quality(rgb, max_sse=qc.U64_MAX // 2).container == good.container
    assert ctx.read_kernel_timing()[1] > 0
    ctx.kernel_timing(False)
    # the other refusals
    for bad in (lambda: ctx.encode_image_quality(rgb, max_sse=10 ** 9, index_interval=7), lambda: ctx.encode_image_quality(rgb, max_sse=10 ** 9, index_interval=1 << 20),
                lambda: ctx.encode_image_quality_device(0, W, H, max_sse=10 ** 9), lambda: ctx.encode_image_quality_device(d_rgb.data_ptr(), 0, H, max_sse=10 ** 9),
                lambda: ctx.encode_image_quality_device(d_rgb.data_ptr(), W, -1, max_sse=10 ** 9), lambda: ctx.encode_image_quality(rgb, psnr=float("nan"))):
        with pytest.raises(ia.MpcError) as e:
            bad()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    info, out, n = ia.api.MpcQualityInfo(), ia.api._u8p(), ia.api.C.c_size_t(0)
    byref, px = ia.api.C.byref, rgb.ctypes.data_as(ia.api.C.c_void_p)
    for args in ((ctx.h, px, W, H, None, 10 ** 9, -1, None, byref(n), None, None, None, byref(info)),
                 (ctx.h, px, W, H, None, 10 ** 9, -1, byref(out), None, None, None, None, byref(info)),
                 (ctx.h, px, W, H, None, 10 ** 9, -1, byref(out), byref(n), None, None, None, None),
                 (ctx.h, px, W, H, None, 10 ** 9, 0, byref(out), byref(n), None, None, None, byref(info)),
                 (None, px, W, H, None, 10 ** 9, -1, byref(out), byref(n), None, None, None, byref(info))):
        assert ctx.L.mpc_encode_image_quality(*args) == ia.api.MPC_ERR_ARGUMENT
    for both in (dict(), dict(psnr=30.0, max_sse=5)):
        with pytest.raises(ValueError):
            ctx.encode_image_quality(rgb, **both)
    host_only = ia.create_compression_context(K, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        host_only.encode_image_quality(rgb, max_sse=10 ** 9)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host_only.close()
    # left as found: the quant tables, the fast flag, the workgroup limit -- also by a call with an override and by a refused one
    override = 2.0 * np.maximum(np.floor(quant), 1.0)
    with_override = ctx.encode_image_quality(rgb, max_sse=qc.U64_MAX // 2, quant=override, index_interval=0)
    assert with_override.container != good.container
    assert np.array_equal(ctx.quant, quant) and ctx.fast == fast
    assert workgroups(ctx.h) == 100
    ctx.set_tile_encode_workgroups(0)
    assert ctx.encode_image(rgb) == full and ctx.encode_image_quality(rgb, max_sse=qc.U64_MAX // 2).container == good.container


# ---- 5. the budget encode returns what it returned before -------------------------------------------------------------------------

def test_budget_encode_returns_the_bytes_of_the_commit_before(ia, oracle):
    with open(os.path.join(GOLDEN, "budget_bytes_parent.json")) as f:
        want = json.load(f)["entries"]
    got = qc.budget_golden(lambda K, fast: _context(ia, K, fast), oracle.synth_frame, hashlib)
    assert sorted(got) == sorted(want) and len(want) == len(qc.FRAMES) * len(qc.FRAME_KS) * 2 * len(qc.BUDGET_QUARTERS)
    for key in sorted(want):
        assert got[key] == want[key], key
    made = [v for v in want.values() if "sha256" in v]
    assert len(made) >= len(want) * 2 // 3 and len({v["sha256"] for v in made}) >= len(made) // 2  # containers, and not all one
    assert any(v["lambda_index"] >= 0 and v["probes"] > 1 for v in made)                          # ... some of them from the search


def test_the_other_cut_encodes_return_the_bytes_of_the_commit_before(ia, oracle):
    """the quality encode, both encodes with an emphasis map in their host and device forms, and the delta stream to a budget, against
    what they returned at the commit in front of their shared front end and search (tests/golden/cut_bytes_parent.json)"""
    import torch

    def to_device(array):
        tensor = torch.from_numpy(array).cuda()
        torch.cuda.synchronize()
        return tensor

    with open(os.path.join(GOLDEN, "cut_bytes_parent.json")) as f:
        want = json.load(f)["entries"]
    got = qc.cut_golden(lambda K, fast: _context(ia, K, fast), oracle.synth_frame, hashlib, to_device)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
    per_frame = len(qc.QUALITY_MULTIPLES) + 2 * len(qc.EMPHASIS_QUARTERS) + 2 + qc.STREAM_FRAMES
    assert len(want) >= len(qc.FRAMES) * len(qc.FRAME_KS) * 2 * per_frame
    for key in want:                                                # the host form and the device form of a call: one result
        if key.endswith(" host"):
            assert want[key] == want[key[:-len("host")] + "device"], key
    made = [v for v in want.values() if "sha256" in v]
    assert len(made) >= -(-len(want) * 2 // 3)                      # containers and patches, not refusals
    assert any(v["lambda_index"] > 0 for k, v in want.items() if " quality " in k and "emphasis" not in k and "sha256" in v)
    assert any(v["probes"] > 1 for k, v in want.items() if " stream " in k and "sha256" in v)
