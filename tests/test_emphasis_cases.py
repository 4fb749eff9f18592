"""Emphasis maps on the host (no GPU): mpc_budget_allocate_emphasis, mpc_budget_sweep_emphasis, mpc_budget_allocate_floor_emphasis and
mpc_emphasis_from_mask against the numpy model of emphasis_cases.py; every wrong variant of the model fails the case named for it; the
neutral map is the plain functions bit for bit; two properties over random maps; the argument refusals."""
import ctypes as C

import numpy as np
import pytest

import budget_cases as bc
import emphasis_cases as ec
import imageexperiments_amd as ia
import rate_cases as rc

CASES, FLOOR_CASES, MASK_CASES = ec.cases(), ec.floor_cases(), ec.mask_cases()


def _same(got, want):
    """(arrays ..., totals) of the library against the model's: arrays equal, totals equal as Python ints"""
    return all(np.array_equal(a, b) for a, b in zip(got[:-1], want[:-1])) and [int(v) for v in got[-1]] == list(want[-1])


@pytest.mark.parametrize("K", ec.KS)
def test_host_allocation_and_sweep_are_the_model(K):
    mine = [c for c in CASES if c[1].shape[1] == K + 1]
    assert len(mine) >= len(ec.TILE_COUNTS) + 8
    for name, P, counts, e, W, js, grid in mine:
        for j in js:
            assert _same(ia.budget_allocate_emphasis(P, counts, e, W, j), ec.allocate(P, counts, e, W, j)), (name, j)
        if P.shape[0] <= 17:
            assert ia.budget_sweep_emphasis(P, counts, e, W).tolist() == ec.sweep(P, counts, e, W), name
        else:                                                        # the two host loops against each other at every multiplier
            S = ia.budget_sweep_emphasis(P, counts, e, W)
            assert all([int(v) for v in S[j]] == [int(v) for v in ia.budget_allocate_emphasis(P, counts, e, W, j)[2]] for j in range(ec.LAMBDAS)), name


def test_at_the_bound_nothing_is_kept_at_the_last_multiplier():
    for name, P, counts, e, W, js, _ in CASES:
        if "at the bound" in name:
            depth, cut, totals = ia.budget_allocate_emphasis(P, counts, e, W, 255)
            assert not depth.any() and not cut.any() and int(totals[0]) == bc.P_MAX * P.shape[0] and int(totals[2]) == 0, name
            assert ia.budget_allocate_emphasis(P, counts, e, W, 200)[0].all(), name     # ... and below it the case is not trivial


def test_host_floor_allocation_is_the_model():
    for name, P, counts, floor, must, e, listed, W, js in FLOOR_CASES:
        for j in js:
            got = ia.budget_allocate_floor_emphasis(P, counts, floor, must, e, listed, W, j)
            assert _same(got, ec.allocate_floor(P, counts, floor, must, e, listed, W, j)), (name, j)


def test_host_mask_is_the_model():
    seen = set()
    for name, buffer, offset, width, height, lo, hi in MASK_CASES:
        before = buffer.copy()
        got = ia.emphasis_from_mask(ec.mask_view(buffer, offset, width, height), lo, hi)
        assert np.array_equal(got, ec.from_mask(buffer, offset, width, height, lo, hi)), name
        assert got.min() >= lo and got.max() <= hi and np.array_equal(buffer, before)
        seen.add((width, height))
    assert seen >= {(w, h) for w in ec.MASK_WIDTHS for h in ec.MASK_HEIGHTS}


@pytest.mark.parametrize("mistake", ec.WRONG_ALLOCATE + ec.WRONG_FLOOR + ec.WRONG_MASK)
def test_every_wrong_variant_fails_its_case(mistake):
    named = ec.CAUGHT_BY[mistake]
    if mistake in ec.WRONG_ALLOCATE:
        name, P, counts, e, W, js, grid = next(c for c in CASES if c[0] == named)
        differs = [ec.allocate(P, counts, e, W, j, mistake, grid) for j in js]
        right = [ec.allocate(P, counts, e, W, j) for j in js]
    elif mistake in ec.WRONG_FLOOR:
        name, P, counts, floor, must, e, listed, W, js = next(c for c in FLOOR_CASES if c[0] == named)
        differs = [ec.allocate_floor(P, counts, floor, must, e, listed, W, j, mistake) for j in js]
        right = [ec.allocate_floor(P, counts, floor, must, e, listed, W, j) for j in js]
    else:
        name, buffer, offset, width, height, lo, hi = next(c for c in MASK_CASES if c[0] == named)
        differs, right = [(ec.from_mask(buffer, offset, width, height, lo, hi, mistake), [])], [(ec.from_mask(buffer, offset, width, height, lo, hi), [])]
    assert any(not _same(a, b) for a, b in zip(differs, right)), (mistake, named)


def test_the_neutral_map_is_the_plain_functions_bit_for_bit():
    for name, P, counts, _, W, js, _ in CASES:
        T = P.shape[0]
        for e in (None, np.full(T, ec.NEUTRAL, np.uint8)):
            for j in js:
                assert _same(ia.budget_allocate_emphasis(P, counts, e, W, j), ia.budget_allocate(P, counts, W, j)), (name, j)
                assert _same(ia.budget_allocate(P, counts, W, j), bc.allocate(P, counts, W, j)), (name, j)
            if T <= 33:
                assert np.array_equal(ia.budget_sweep_emphasis(P, counts, e, W), ia.budget_sweep(P, counts, W)), name
    for name, P, counts, floor, must, e, listed, W, js in FLOOR_CASES:
        for j in js:
            plain = ia.budget_allocate_floor(P, counts, floor, must, W, j)
            assert _same(plain, rc.allocate_floor(P, counts, floor, must, W, j)), (name, j)
            assert _same(ia.budget_allocate_floor_emphasis(P, counts, floor, must, None, listed, W, j), plain), (name, j)
            assert _same(ia.budget_allocate_floor_emphasis(P, counts, floor, must, np.full(len(e), ec.NEUTRAL, np.uint8), listed, W, j), plain), (name, j)


def test_a_tile_whose_emphasis_rises_never_ends_worse_and_one_whose_falls_never_better():
    rng = np.random.default_rng(7)
    for K in ec.KS:
        _, P, counts, _, W, _, _ = ec._random_case(rng, K, 200)
        rows, moved = np.arange(P.shape[0]), False
        for j in (1, 60, 113, 160, 220):
            base = P[rows, ia.budget_allocate(P, counts, W, j)[0]].astype(np.int64)
            e = ec._random_map(rng, P.shape[0])
            got = P[rows, ia.budget_allocate_emphasis(P, counts, e, W, j)[0]].astype(np.int64)
            u = ec.used(e)
            assert (got[u > ec.NEUTRAL] <= base[u > ec.NEUTRAL]).all() and (got[u < ec.NEUTRAL] >= base[u < ec.NEUTRAL]).all(), (K, j)
            assert np.array_equal(got[u == ec.NEUTRAL], base[u == ec.NEUTRAL])
            moved = moved or bool((got != base).any())
        assert moved, K                                              # the maps did move tiles: the property is not vacuous


def test_along_the_ladder_the_true_error_never_falls_and_the_rate_never_rises():
    rng = np.random.default_rng(8)
    for K in ec.KS:
        for _ in range(3):
            _, P, counts, e, W, _, _ = ec._random_case(rng, K, 120)
            S = ia.budget_sweep_emphasis(P, counts, e, W).astype(object)
            assert all(a <= b for a, b in zip(S[:, 0], S[1:, 0])) and all(a >= b for a, b in zip(S[:, 1], S[1:, 1])), K
            assert S[0, 0] < S[255, 0] and ia.quality_pick(S.astype(np.uint64), int(S[100, 0])) >= 100


def test_argument_refusals():
    L = ia.load_library()
    K, T = 5, 4
    P, counts, W = np.zeros((T, K + 1), np.uint32), np.zeros((T, 3), np.uint16), np.full((3, K), 1000, np.uint32)
    e, depth, cut, send = np.full(T, 16, np.uint8), np.zeros(T, np.uint8), np.zeros((T, 3), np.uint16), np.zeros(T, np.uint8)
    totals = np.zeros(768, np.uint64)
    u8, u16, u32, u64, i32 = (C.POINTER(t) for t in (C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_int32))
    p, c, w, ep, tp = P.ctypes.data_as(u32), counts.ctypes.data_as(u16), W.ctypes.data_as(u32), e.ctypes.data_as(u8), totals.ctypes.data_as(u64)
    dp, cp, sp = depth.ctypes.data_as(u8), cut.ctypes.data_as(u16), send.ctypes.data_as(u8)
    ARG = ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_budget_allocate_emphasis(p, c, ep, T, K, w, 0, dp, cp, tp) == 0 and L.mpc_budget_allocate_emphasis(p, c, None, T, K, w, 0, None, None, tp) == 0
    for args in ((None, c, ep, T, K, w, 0, dp, cp, tp), (p, None, ep, T, K, w, 0, dp, cp, tp), (p, c, ep, T, K, None, 0, dp, cp, tp),
                 (p, c, ep, T, K, w, 0, dp, cp, None), (p, c, ep, -1, K, w, 0, dp, cp, tp), (p, c, ep, T, 0, w, 0, dp, cp, tp),
                 (p, c, ep, T, 33, w, 0, dp, cp, tp), (p, c, ep, T, K, w, -1, dp, cp, tp), (p, c, ep, T, K, w, 256, dp, cp, tp)):
        assert L.mpc_budget_allocate_emphasis(*args) == ARG, args
    assert L.mpc_budget_sweep_emphasis(p, c, ep, T, K, w, tp) == 0 and L.mpc_budget_sweep_emphasis(p, c, None, 0, K, w, tp) == 0
    for args in ((None, c, ep, T, K, w, tp), (p, None, ep, T, K, w, tp), (p, c, ep, T, K, None, tp), (p, c, ep, T, K, w, None),
                 (p, c, ep, -1, K, w, tp), (p, c, ep, T, 0, w, tp), (p, c, ep, T, 33, w, tp)):
        assert L.mpc_budget_sweep_emphasis(*args) == ARG, args
    lp = np.arange(T, dtype=np.int32).ctypes.data_as(i32)
    ok = (p, c, None, None, ep, lp, T, T, K, w, 0, dp, cp, sp, tp)
    assert L.mpc_budget_allocate_floor_emphasis(*ok) == 0

    def but(**kw):
        names = ("profile", "counts", "floor", "must", "emphasis", "list", "tiles", "n", "K", "weights", "j", "depth", "cut", "send", "totals")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    for args in (but(profile=None), but(counts=None), but(weights=None), but(totals=None), but(n=-1), but(K=0), but(K=33), but(j=-1), but(j=256),
                 but(tiles=0), but(tiles=-3), but(list=None, tiles=T - 1)):
        assert L.mpc_budget_allocate_floor_emphasis(*args) == ARG, args
    assert L.mpc_budget_allocate_floor_emphasis(*but(emphasis=None, tiles=0, list=None)) == 0        # no map: the tile count is not looked at
    mask, out = np.zeros((9, 20), np.uint8), np.zeros(6, np.uint8)
    mp, op = C.c_void_p(mask.ctypes.data), out.ctypes.data_as(u8)
    assert L.mpc_emphasis_from_mask(mp, 20, 9, 20, 1, 64, op) == 0
    for args in ((None, 20, 9, 20, 1, 64, op), (mp, 20, 9, 20, 1, 64, None), (mp, 0, 9, 20, 1, 64, op), (mp, 20, 0, 20, 1, 64, op),
                 (mp, 20, -1, 20, 1, 64, op), (mp, 20, 9, 19, 1, 64, op), (mp, 20, 9, 20, 0, 64, op), (mp, 20, 9, 20, 1, 65, op),
                 (mp, 20, 9, 20, 17, 16, op), (mp, 1 << 30, 1 << 30, 1 << 30, 1, 64, op)):
        assert L.mpc_emphasis_from_mask(*args) == ARG, args
    with pytest.raises(ValueError):
        ia.budget_allocate_emphasis(P, counts, np.zeros(T + 1, np.uint8), W, 0)
    with pytest.raises(ValueError):
        ia.emphasis_from_mask(np.zeros((4, 4), np.int32))
    # the device forms refuse a host-only context
    ctx = ia.create_compression_context(K, 8, 3.5, device=-1)
    for call in (lambda: ctx.budget_allocate_emphasis_device(1, 1, 1, T, W, 0, 1, 1, 1), lambda: ctx.budget_sweep_emphasis_device(1, 1, 1, T, W, 1),
                 lambda: ctx.budget_allocate_floor_emphasis_device(1, 1, 0, 0, 1, 0, T, T, W, 0, 1, 1, 1, 1),
                 lambda: ctx.emphasis_from_mask_device(1, 20, 9, 1), lambda: ctx.encode_image_budget_emphasis(np.zeros((8, 8, 3), np.uint8), 100, [16]),
                 lambda: ctx.encode_image_quality_emphasis(np.zeros((8, 8, 3), np.uint8), [16], max_sse=5)):
        with pytest.raises(ia.MpcError) as err:
            call()
        assert err.value.status == ia.api.MPC_ERR_NO_DEVICE
    ctx.close()
