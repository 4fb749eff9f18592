"""The target-quality encode on the host: mpc_budget_sweep, mpc_quality_pick and mpc_sse_for_psnr against the numpy model of
tests/quality_cases.py on every case, the model against budget_cases.allocate, the cases against the mistakes they are there to
catch, the monotonicity the pick rests on, refusals.  No GPU."""
import math

import numpy as np
import pytest

import budget_cases as bc
import quality_cases as qc

CASES = qc.cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def model():
    """the model's sweep of every case, once"""
    return {name: qc.sweep(P, counts, W) for name, P, counts, W in CASES}


def test_the_cases_cover_what_the_contract_names():
    assert len(set(IDS)) == len(IDS) and set(c[0] for c in bc.cases()) <= set(IDS)
    for K in (1, 8, 32):
        for T in (1, 3, 4, 5, 257):
            name, P, counts, W = next(c for c in CASES if c[0] == f"K{K} T{T} quality")
            assert P.shape == (T, K + 1) and (counts == 0).any() and (counts == K + 1).any()
            if K > 1 and T > 1:
                assert (np.diff(P.astype(np.int64), axis=1) > 0).any(), name       # not monotone in depth
    for name, P, counts, W in CASES:
        assert P.dtype == np.uint32 and counts.dtype == np.uint16 and W.dtype == np.uint32
        assert P.shape == (counts.shape[0], W.shape[1] + 1) and int(P.max()) <= bc.P_MAX
        assert int(W.min()) >= bc.W_MIN and int(W.max()) <= bc.W_MAX
    name, P, counts, W = next(c for c in CASES if c[0] == "K32 largest J")
    largest = bc.P_MAX * 65536 + bc.lambda_of(255) * int(bc.rates(counts, W, 32).max())
    assert int(P.max()) == bc.P_MAX and (W == bc.W_MAX).all() and 1 << 61 < largest < 1 << 64


def test_a_distortion_total_exceeds_32_bits(model):
    S = model["K1 T400 above 2^32"]
    assert S[255][0] > 1 << 32 and S[0][0] < S[255][0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_model_is_allocate_at_each_j(case, model):
    """the vectorised sweep against budget_cases.allocate: at every j where that is quick, at a spread of j elsewhere"""
    name, P, counts, W = case
    T, K = P.shape[0], P.shape[1] - 1
    js = range(qc.LAMBDAS) if T * (K + 1) <= 65 * 9 else (0, 1, 2, 9, 40, 77, 90, 120, 121, 129, 160, 200, 254, 255)
    want = qc.sweep_by_allocate(P, counts, W, js)
    for j in js:
        assert model[name][j] == want[j], (name, j)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_is_the_model_and_the_allocation_at_every_j(ia, case, model):
    name, P, counts, W = case
    S = ia.budget_sweep(P, counts, W)
    assert S.dtype == np.uint64 and S.shape == (qc.LAMBDAS, 3)
    assert [[int(v) for v in row] for row in S] == model[name], name
    for j in range(qc.LAMBDAS):
        totals = ia.budget_allocate(P, counts, W, j)[2]
        assert [int(v) for v in totals] == [int(v) for v in S[j]], (name, j)
    assert S[255][1] == 0 and S[255][2] == 0                                     # at j = 255 every depth is 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_distortion_rises_and_rate_falls_along_the_ladder(case, model):
    S = model[case[0]]
    assert all(S[j][0] <= S[j + 1][0] and S[j][1] >= S[j + 1][1] for j in range(qc.LAMBDAS - 1)), case[0]
    assert S[0][0] == int(case[1].min(axis=1).astype(np.int64).sum())            # D[0]: each tile's least profile entry


@pytest.mark.parametrize("mistake", qc.WRONG_SWEEP)
def test_the_cases_tell_the_model_from_a_wrong_sweep(mistake, model):
    caught = [name for name, P, counts, W in CASES if qc.sweep(P, counts, W, mistake) != model[name]]
    assert caught, mistake


@pytest.mark.parametrize("mistake", qc.WRONG_PICK)
def test_the_cases_tell_the_pick_from_a_wrong_pick(mistake, model):
    caught = [name for name in IDS if any(qc.pick(model[name], s, mistake) != qc.pick(model[name], s) for s in qc.pick_targets(model[name]))]
    assert caught, mistake


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pick_is_the_model(ia, case, model):
    name = case[0]
    S = model[name]
    totals = np.array(S, np.uint64)
    targets = qc.pick_targets(S)
    assert {0, qc.U64_MAX, S[0][0], S[255][0]} <= set(targets) and (S[0][0] == 0 or S[0][0] - 1 in targets)
    for s in targets:
        got = ia.quality_pick(totals, s)
        assert got == qc.pick(S, s), (name, s)
        assert got == max((j for j in range(qc.LAMBDAS) if S[j][0] <= s), default=-1)
    assert ia.quality_pick(totals, qc.U64_MAX) == 255 and ia.quality_pick(totals, S[0][0]) >= 0
    if S[0][0] > 0:
        assert ia.quality_pick(totals, S[0][0] - 1) == -1 and ia.quality_pick(totals, 0) == -1


def test_pick_holds_to_its_definition_where_the_totals_are_not_monotone(ia):
    """the largest j, not a bisection's: totals no sweep makes"""
    totals = np.zeros((256, 3), np.uint64)
    totals[:, 0] = 1000
    totals[17, 0] = 10
    totals[200, 0] = 20
    assert ia.quality_pick(totals, 9) == -1 and ia.quality_pick(totals, 10) == 17 and ia.quality_pick(totals, 25) == 200
    assert ia.quality_pick(totals, 1000) == 255


# ---- mpc_sse_for_psnr ----

GEOMETRIES = ((64, 48), (197, 117), (1, 1))


def _frames_with_sse(s, W, H):
    """two frames of W x H whose squared difference is exactly s, or None where the frame is too small for it"""
    a, b = np.zeros(H * W * 3, np.uint8), np.zeros(H * W * 3, np.uint8)
    at = 0
    while s:
        d = min(255, math.isqrt(s))
        if at == a.size:
            return None
        b[at] = d
        s -= d * d
        at += 1
    return a.reshape(H, W, 3), b.reshape(H, W, 3)


def _psnr(ia, s, W, H):
    frames = _frames_with_sse(s, W, H)
    return None if frames is None else ia.calculate_psnr(*frames)


@pytest.mark.parametrize("W,H", GEOMETRIES)
def test_sse_for_psnr_round_trips_against_mpc_psnr(ia, W, H):
    tiles = -(-W // 8) * -(-H // 8)
    limit = 195075 * 64 * tiles
    room = 255 * 255 * 3 * W * H                                     # what two frames of this size can differ by
    spread = sorted({1, 2, 3, 7, 100, 65025, 65026, 195075, room // 3, room // 2 + 1, room - 1, room} - {0})
    seen = 0
    for s in spread:
        here, above = _psnr(ia, s, W, H), _psnr(ia, s + 1, W, H)
        if here is None:
            continue
        got = ia.sse_for_psnr(here, W, H)
        assert s <= got <= limit, (s, got)
        assert _psnr(ia, got, W, H) >= here                         # the answer reaches the target, to the bit
        if above is not None and above < here:
            assert got == s, (s, got)                               # ... and s + 1 does not: s is the largest
            assert ia.sse_for_psnr(math.nextafter(here, math.inf), W, H) < s
        seen += 1
    assert seen >= 6
    assert ia.sse_for_psnr(math.inf, W, H) == 0 and _psnr(ia, 0, W, H) == math.inf
    assert ia.sse_for_psnr(1e300, W, H) == 0                        # no s but 0 is that good
    assert ia.sse_for_psnr(-1e300, W, H) == limit                   # every s of the range is
    assert ia.sse_for_psnr(ia.calculate_psnr(*_frames_with_sse(1, W, H)), W, H) == 1


def test_sse_for_psnr_falls_as_the_target_rises(ia):
    got = [ia.sse_for_psnr(p, 1920, 1080) for p in (10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 90.0)]
    assert all(a > b for a, b in zip(got, got[1:])) and got[-1] >= 0
    # 10 dB is a factor of ten in the squared error
    assert abs(got[1] / got[2] - 10.0) < 1e-3


def test_refusals(ia):
    L, C = ia.load_library(), ia.api.C
    u32, u16, u64 = ia.api._u32p, ia.api._u16p, C.POINTER(C.c_uint64)
    P, c, W, S = np.zeros(9, np.uint32), np.zeros(3, np.uint16), np.full(24, 256, np.uint32), np.zeros(768, np.uint64)
    ok = lambda tiles, K: L.mpc_budget_sweep(P.ctypes.data_as(u32), c.ctypes.data_as(u16), tiles, K, W.ctypes.data_as(u32), S.ctypes.data_as(u64))
    assert ok(1, 8) == ia.api.MPC_OK and ok(0, 8) == ia.api.MPC_OK and not S.any()          # no tiles is no work: all 768 words are 0
    for tiles, K in ((-1, 8), (1, 0), (1, 33), (1, -1)):                                   # what mpc_budget_allocate refuses
        assert ok(tiles, K) == ia.api.MPC_ERR_ARGUMENT
    args = [P.ctypes.data_as(u32), c.ctypes.data_as(u16), 1, 8, W.ctypes.data_as(u32), S.ctypes.data_as(u64)]
    for null in (0, 1, 4, 5):
        assert L.mpc_budget_sweep(*[None if k == null else a for k, a in enumerate(args)]) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_quality_pick(None, 5) == -1
    out = C.c_uint64(77)
    for psnr, w, h in ((math.nan, 64, 48), (-math.inf, 64, 48), (30.0, 0, 48), (30.0, 64, 0), (30.0, -3, 5), (30.0, 1 << 20, 1 << 20)):
        assert L.mpc_sse_for_psnr(psnr, w, h, C.byref(out)) == ia.api.MPC_ERR_ARGUMENT, (psnr, w, h)
    assert L.mpc_sse_for_psnr(30.0, 64, 48, None) == ia.api.MPC_ERR_ARGUMENT
    for bad in (math.nan, -math.inf):
        with pytest.raises(ia.MpcError) as e:
            ia.sse_for_psnr(bad, 64, 48)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
