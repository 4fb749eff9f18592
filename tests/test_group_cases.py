"""A group of frames on the host (no GPU): mpc_budget_allocate_group and mpc_budget_sweep_group against the numpy model of
group_cases.py and against the single-frame host functions frame by frame; the model against budget_cases.allocate; every wrong variant
of the model is told apart by the cases of every K, with and without a map; mpc_sse_for_psnr_group; the argument refusals."""
import ctypes as C
import math

import numpy as np
import pytest

import budget_cases as bc
import group_cases as gc
import imageexperiments_amd as ia

CASES = gc.cases()


def _of(K):
    return [c for c in CASES if c[1].shape[2] == K + 1]


def _maps(E):
    return (("map", E), ("no map", None))


def test_the_cases_cover_what_they_claim():
    assert len(CASES) == len(gc.KS) * len(gc.FRAME_COUNTS) * len(gc.TILE_COUNTS)
    assert {c[1].shape[0] for c in CASES} == set(gc.FRAME_COUNTS) and {c[1].shape[1] for c in CASES} == set(gc.TILE_COUNTS)
    assert max(gc.FRAME_COUNTS) > gc.CHUNK and gc.CHUNK in (8,)
    for K in gc.KS:
        mine = _of(K)
        assert any(c[2].shape[0] > 1 and not c[2][1].any() for c in mine)                   # a frame with all counts 0
        assert any(int(c[2].max()) > K for c in mine)                                       # counts above K
        assert all({0, 1, 16, 64, 255} <= set(c[3].reshape(-1).tolist()) for c in mine if c[3].size >= 25)
        for c in mine:                                                                      # weights apart by octaves, inside the clamp
            W = c[4].astype(np.int64)
            assert W.min() >= bc.W_MIN and W.max() <= bc.W_MAX
            assert all(not np.array_equal(W[f], W[f + 1]) for f in range(W.shape[0] - 1))


@pytest.mark.parametrize("K", gc.KS)
def test_host_group_allocation_is_the_model_and_the_single_frame_function(K):
    for name, P, counts, E, W, js in _of(K):
        F = P.shape[0]
        for label, e in _maps(E):
            for j in js:
                depth, cut, totals = ia.budget_allocate_group(P, counts, e, W, j)
                want = gc.allocate_group(P, counts, e, W, j)
                assert np.array_equal(depth, want[0]) and np.array_equal(cut, want[1]), (name, label, j)
                assert [[int(v) for v in row] for row in totals] == want[2], (name, label, j)
                for f in range(F):
                    d1, c1, t1 = ia.budget_allocate_emphasis(P[f], counts[f], None if e is None else e[f], W[f], j)
                    assert np.array_equal(depth[f], d1) and np.array_equal(cut[f], c1) and np.array_equal(totals[f], t1), (name, label, j, f)


@pytest.mark.parametrize("K", gc.KS)
def test_host_group_sweep_is_the_model_and_the_sum_of_the_single_frame_sweeps(K):
    for name, P, counts, E, W, js in _of(K):
        F = P.shape[0]
        for label, e in _maps(E):
            S = ia.budget_sweep_group(P, counts, e, W)
            assert S.shape == (gc.LAMBDAS, 3)
            want = gc.sweep_group(P, counts, e, W, js=js)
            for j in js:
                assert [int(v) for v in S[j]] == want[j], (name, label, j)
            frames = sum(ia.budget_sweep_emphasis(P[f], counts[f], None if e is None else e[f], W[f]) for f in range(F))
            assert np.array_equal(S, frames), (name, label)
            # the two group loops against each other at every multiplier
            if F * P.shape[1] <= 75:
                for j in range(gc.LAMBDAS):
                    assert np.array_equal(S[j], ia.budget_allocate_group(P, counts, e, W, j)[2].sum(axis=0)), (name, label, j)
            D = [int(v) for v in S[:, 0]]
            assert all(a <= b for a, b in zip(D, D[1:])), (name, label)                     # the pick's premise holds for the sum


def test_the_model_without_a_map_is_budget_cases_allocate_frame_by_frame():
    for name, P, counts, E, W, js in CASES:
        if P.shape[0] * P.shape[1] > 51:
            continue
        for j in js:
            depth, cut, totals = gc.allocate_group(P, counts, None, W, j)
            for f in range(P.shape[0]):
                d1, c1, t1 = bc.allocate(P[f], counts[f], W[f], j)
                assert np.array_equal(depth[f], d1) and np.array_equal(cut[f], c1) and totals[f] == [int(v) for v in t1], (name, j, f)


@pytest.mark.parametrize("mistake", gc.WRONG)
def test_every_wrong_variant_is_told_apart_by_the_cases_of_every_K(mistake):
    for K in gc.KS:
        for with_map in (True,) if mistake in gc.NEEDS_MAP else (True, False):
            caught = [c[0] for c in _of(K) if c[1].shape[0] > 1 and gc.told_apart(c, mistake, with_map)]
            assert caught, (mistake, K, with_map)
            # and the library is on the model's side there
            name, P, counts, E, W, js = next(c for c in _of(K) if c[0] == caught[0])
            e = E if with_map else None
            if mistake == "sweep without the last frame":
                S = ia.budget_sweep_group(P, counts, e, W)
                bad = gc.sweep_group(P, counts, e, W, mistake, js=js)
                assert any([int(v) for v in S[j]] != bad[j] for j in js), (mistake, name)
            else:
                differs = False
                for j in js:
                    depth, cut, totals = ia.budget_allocate_group(P, counts, e, W, j)
                    bad = gc.allocate_group(P, counts, e, W, j, mistake)
                    differs |= not (np.array_equal(depth, bad[0]) and np.array_equal(cut, bad[1]) and [[int(v) for v in r] for r in totals] == bad[2])
                assert differs, (mistake, name)


def test_a_run_that_crosses_a_frame_boundary_is_told_apart_wherever_there_is_one():
    """every case of more than one frame and at least 15 tiles a frame whose tile count is no multiple of the run"""
    for mistake, run in (("a 16-tile run continues into the next frame", 16), ("a 4-tile workgroup continues into the next frame", 4)):
        mine = [c for c in CASES if c[1].shape[0] > 1 and c[1].shape[1] >= 15 and c[1].shape[1] % run]
        assert len(mine) >= 20
        missed = [c[0] for c in mine if not gc.told_apart(c, mistake, False)]
        assert not missed, (mistake, missed)


def test_one_frame_is_the_single_frame_function_and_a_neutral_map_is_no_map():
    for name, P, counts, E, W, js in CASES:
        if P.shape[0] == 1:
            for j in js:
                got, want = ia.budget_allocate_group(P, counts, E, W, j), ia.budget_allocate_emphasis(P[0], counts[0], E[0], W[0], j)
                assert all(np.array_equal(a[0], b) for a, b in zip(got, want)), (name, j)
            assert np.array_equal(ia.budget_sweep_group(P, counts, None, W), ia.budget_sweep(P[0], counts[0], W[0])), name
        neutral = np.full(E.shape, 16, np.uint8)
        assert np.array_equal(ia.budget_sweep_group(P, counts, neutral, W), ia.budget_sweep_group(P, counts, None, W)), name
        for j in js[::3]:
            a, b = ia.budget_allocate_group(P, counts, neutral, W, j), ia.budget_allocate_group(P, counts, None, W, j)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (name, j)


def test_sse_for_psnr_group():
    def psnr(s, pixels):
        return math.inf if s == 0 else 20.0 * math.log10(765.0) - 10.0 * math.log10(s / pixels)

    for W, H in ((1, 1), (64, 48), (197, 117), (1920, 1080)):
        tiles = -(-W // 8) * -(-H // 8)
        for target in (math.inf, 99.0, 48.13, 35.5, 30.0, 20.0, 1.0, 0.0, -5.0, -1e300):
            assert ia.sse_for_psnr_group(target, W, H, 1) == ia.sse_for_psnr(target, W, H)
            last = None
            for frames in (1, 2, 3, 9, 64):
                s, limit = ia.sse_for_psnr_group(target, W, H, frames), 195075 * 64 * tiles * frames
                assert 0 <= s <= limit
                # the largest s with psnr(s) >= target, by the formula itself up to a rounding of the logarithm
                assert psnr(s, frames * W * H) >= target - 1e-9 and (s == limit or psnr(s + 1, frames * W * H) < target + 1e-9), (W, H, target, frames, s)
                assert last is None or s >= last
                last = s
    u64 = C.c_uint64(0)
    L = ia.load_library()
    ARG = ia.api.MPC_ERR_ARGUMENT
    for args in ((float("nan"), 64, 48, 2, C.byref(u64)), (-math.inf, 64, 48, 2, C.byref(u64)), (30.0, 0, 48, 2, C.byref(u64)), (30.0, 64, -1, 2, C.byref(u64)),
                 (30.0, 64, 48, 0, C.byref(u64)), (30.0, 64, 48, 65, C.byref(u64)), (30.0, 64, 48, -3, C.byref(u64)), (30.0, 64, 48, 2, None)):
        assert L.mpc_sse_for_psnr_group(*args) == ARG, args
    assert L.mpc_sse_for_psnr_group(30.0, 64, 48, 64, C.byref(u64)) == 0


def test_argument_refusals():
    L = ia.load_library()
    K, T, F = 5, 4, 3
    P, counts, W = np.zeros((F, T, K + 1), np.uint32), np.zeros((F, T, 3), np.uint16), np.full((F, 3, K), 1000, np.uint32)
    e, depth, cut = np.full((F, T), 16, np.uint8), np.zeros((F, T), np.uint8), np.zeros((F, T, 3), np.uint16)
    totals = np.zeros(768, np.uint64)
    u8, u16, u32, u64 = (C.POINTER(t) for t in (C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64))
    p, c, w, ep, tp = P.ctypes.data_as(u32), counts.ctypes.data_as(u16), W.ctypes.data_as(u32), e.ctypes.data_as(u8), totals.ctypes.data_as(u64)
    dp, cp = depth.ctypes.data_as(u8), cut.ctypes.data_as(u16)
    ARG = ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_budget_allocate_group(p, c, ep, F, T, K, w, 0, dp, cp, tp) == 0 and L.mpc_budget_allocate_group(p, c, None, F, T, K, w, 0, None, None, tp) == 0
    assert L.mpc_budget_allocate_group(p, c, None, F, 0, K, w, 0, None, None, tp) == 0
    for args in ((None, c, ep, F, T, K, w, 0, dp, cp, tp), (p, None, ep, F, T, K, w, 0, dp, cp, tp), (p, c, ep, F, T, K, None, 0, dp, cp, tp),
                 (p, c, ep, F, T, K, w, 0, dp, cp, None), (p, c, ep, F, -1, K, w, 0, dp, cp, tp), (p, c, ep, F, T, 0, w, 0, dp, cp, tp),
                 (p, c, ep, F, T, 33, w, 0, dp, cp, tp), (p, c, ep, F, T, K, w, -1, dp, cp, tp), (p, c, ep, F, T, K, w, 256, dp, cp, tp),
                 (p, c, ep, 0, T, K, w, 0, dp, cp, tp), (p, c, ep, 65, T, K, w, 0, dp, cp, tp), (p, c, ep, -1, T, K, w, 0, dp, cp, tp)):
        assert L.mpc_budget_allocate_group(*args) == ARG, args
    assert L.mpc_budget_sweep_group(p, c, ep, F, T, K, w, tp) == 0 and L.mpc_budget_sweep_group(p, c, None, F, 0, K, w, tp) == 0
    for args in ((None, c, ep, F, T, K, w, tp), (p, None, ep, F, T, K, w, tp), (p, c, ep, F, T, K, None, tp), (p, c, ep, F, T, K, w, None),
                 (p, c, ep, F, -1, K, w, tp), (p, c, ep, F, T, 0, w, tp), (p, c, ep, F, T, 33, w, tp), (p, c, ep, 0, T, K, w, tp),
                 (p, c, ep, 65, T, K, w, tp)):
        assert L.mpc_budget_sweep_group(*args) == ARG, args
    big = 64
    Pb, cb, Wb = np.zeros((big, 1, K + 1), np.uint32), np.zeros((big, 1, 3), np.uint16), np.full((big, 3, K), 300, np.uint32)
    assert ia.budget_allocate_group(Pb, cb, None, Wb, 7)[2].shape == (big, 3) and not ia.budget_sweep_group(Pb, cb, None, Wb).any()
    with pytest.raises(ValueError):
        ia.budget_allocate_group(P, counts, np.zeros(F * T + 1, np.uint8), W, 0)
    # the device forms and the calls refuse a host-only context, and before that what needs no device
    ctx = ia.create_compression_context(K, 8, 3.5, device=-1)
    frame = np.zeros((8, 8, 3), np.uint8)
    for call in (lambda: ctx.budget_allocate_group_device(1, 1, 0, F, T, W, 0, 1, 1, 1), lambda: ctx.budget_sweep_group_device(1, 1, 0, F, T, W, 1),
                 lambda: ctx.encode_images_budget([frame, frame], 100), lambda: ctx.encode_images_quality([frame, frame], max_sse=5),
                 lambda: ctx.encode_images_budget_device([1, 1], 8, 8, 100), lambda: ctx.encode_images_quality_device([1, 1], 8, 8, psnr=30.0)):
        with pytest.raises(ia.MpcError) as err:
            call()
        assert err.value.status == ia.api.MPC_ERR_NO_DEVICE
    for call in (lambda: ctx.encode_images_budget([], 100), lambda: ctx.encode_images_budget([frame] * 65, 100),
                 lambda: ctx.encode_images_quality_device([1, 0], 8, 8, max_sse=5), lambda: ctx.encode_images_budget([frame], 0)):
        with pytest.raises(ia.MpcError) as err:
            call()
        assert err.value.status == ARG
    for both in (dict(), dict(psnr=30.0, max_sse=5)):
        with pytest.raises(ValueError):
            ctx.encode_images_quality([frame], **both)
    ctx.close()
