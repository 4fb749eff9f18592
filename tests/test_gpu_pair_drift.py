"""The kept pair approximations of the pursuit kernel, read out of its scratch (run with -m gpu).

The kernel keeps 64 float approximations P_b per pair (a tile-channel and a detail block it has unlocked), started by the screen's
MFMAs and updated with the Gram table after every step, and a bound E per pair that the survivor test relies on
(tests/pair_drift_cases.py has the whole story and the inputs; tests/test_pair_drift_cases.py proves the inputs and the host replay
from the oracle alone).  A wrong P_b or a bound that does not hold changes no record until the true winner happens to sit in the
pair, so bit parity of the records cannot see them.  Here the scratch is filled (mpc_debug_pair_scratch), one calc_mp call of 16
vectors -- one wave's slots -- is stopped at a chosen depth by a 1e30 quantiser, and the scratch is read back.  For every group,
flavour, channel, stop depth and both fill words (all ones, all zeros):

  records      counts, records 0 .. count and swept rows are the oracle's at that quantiser;
  bookkeeping  exactly one wave has touched its scratch; in slot s the pairs with a written E are the replay's of vector s, in
               creation order, word 0 of pair_meta is block | rows << 9 | first dictionary index << 16, and every other word of
               the three arrays still holds the fill word;
  bound        E is within (u + 1) 2^-22 relative of the float64 model after u updates: the start 2^-13 |r~| + 2^-100
               (screen_cases.reference_bound, 2 ulp as in test_gpu_screen_tables.py), then E = (E + 2^-21 (|c32| + |r~|)) 1.000001f
               with |r~| of the residual entering the step -- three float roundings of 2^-24 per update, contracted or not;
  invariant    |P_b - exact_b| <= E for the 62 real rows of every pair, exact = the flavour's chain dot product of the row with
               the residual at the stop (float64, or float32 on the rows rounded to float); rows 62 and 63 are exactly 0;
  values       P is bit for bit the probe's MFMA start (mpc_debug_screen_probe_device on r_{k+1}, the same screen_operands and
               tile_mfma) followed by exact float fused multiply-adds with the resident Gram values (mpc_debug_copy_gram_device);
  no stale     the two fills give bit-identical P, E and meta for the pairs made.

Nothing tighter than 1 is asserted of |P - exact| / E.  Measured on an MI355X, worst ratio per group over channels 0 and 2 and all
depths, double / float flavour (also in DESIGN.md 3):
ramp 0.030 / 0.026; deep 0.023 / 0.024; mixed 0.027 / 0.027; one 0.034 / 0.019; with_row0 0.029 / 0.030; deep_up and deep_down as deep.
A host model of the updates alone (start = the float64 product rounded to float, Gram values = float64 products rounded to float,
the same FMAs and recurrence) gives 3.6e-4 to 4.6e-4 (double flavour) and 4.8e-4 to 5.4e-4 (float flavour, which adds the float
chain's own rounding) at depth 31 on deep, ramp and mixed, channel 0; the device adds the MFMA start's share, at most 0.06 of E_b
(test_gpu_screen_tables.py)."""
import ctypes as C

import numpy as np
import pytest

import pair_drift_cases as pdc

pytestmark = pytest.mark.gpu

FILLS = (0xFFFFFFFF, 0x00000000)
WAVES = 16                         # scratch waves of one workgroup (the kernel runs 12 of them)
N_COLS = pdc.NUM_BASE * 64


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    return torch


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd
    return imageexperiments_amd


@pytest.fixture(scope="module")
def ctx(ia, torch):
    c = ia.create_compression_context(pdc.K, 8, 3.5, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracles(oracle, octx32):
    return {"double": octx32, "float": oracle.OracleFastContext(octx32)}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mfma_start(torch, ctx, ch, blk, r):
    """the 64 approximations a new pair of block `blk` starts with from residual r, and the probe's bound"""
    v = torch.from_numpy(np.ascontiguousarray(r, np.float64).reshape(1, 64)).cuda()
    approx = torch.zeros((1, 576), dtype=torch.float32, device="cuda")
    bound = torch.zeros((1,), dtype=torch.float32, device="cuda")
    ctx.debug_screen_probe_device(ch, blk, v.data_ptr(), 1, approx.data_ptr(), bound.data_ptr())
    torch.cuda.synchronize()
    return approx.cpu().numpy()[0, 512:], float(bound.cpu().numpy()[0])


def expected_values(torch, ctx, ch, rp):
    """end step e -> float32 [pairs created before e, 64]: the P of the vector's pairs when its pursuit ends at step e"""
    ends = sorted({rp.end(d) for d in pdc.DEPTHS})
    if not rp.pairs:
        return {e: np.zeros((0, 64), np.float32) for e in ends}
    P = np.array([mfma_start(torch, ctx, ch, p.block, rp.r[p.created + 1])[0] for p in rp.pairs])
    steps = list(range(1, rp.count))
    G = np.zeros((0, len(rp.pairs), 64), np.float32)
    if steps:
        rows = torch.zeros((len(steps), N_COLS), dtype=torch.float32, device="cuda")
        for n, j in enumerate(steps):                                   # Gram row of the atom of step j
            ctx.debug_copy_gram_device(ch, rp.sel[j], 1, 0, N_COLS, rows[n].data_ptr())
        cols = torch.from_numpy(np.concatenate([64 * p.block + np.arange(64) for p in rp.pairs])).cuda()
        torch.cuda.synchronize()
        G = rows[:, cols].cpu().numpy().reshape(len(steps), len(rp.pairs), 64)
    created = np.array([p.created for p in rp.pairs])
    out = {}
    for j in range(1, rp.count + 1):
        if j in ends:
            out[j] = P[created < j].copy()                             # updated by the steps before j
        if j < rp.count:
            held = created < j                                         # the pair step j itself creates starts from r_{j+1}
            if held.any():
                P[held] = pdc.fma32(-np.float32(rp.c[j]), G[j - 1][held], P[held])
    out.setdefault(0, np.zeros((0, 64), np.float32))
    return out


def run_stopped(ctx, ch, v, depth, fill):
    before = ctx.debug_pair_scratch(0, WAVES, fill)
    assert all((u32(a) == fill).all() for a in before)                 # the fill is what the copy shows
    out = ctx.calc_mp(ch, v, quant_k=pdc.group_quant(v, depth))
    return out, ctx.debug_pair_scratch(0, WAVES)


@pytest.mark.parametrize("channel", pdc.CHANNELS)
@pytest.mark.parametrize("flavour", pdc.FLAVOURS)
@pytest.mark.parametrize("name", pdc.GROUPS)
def test_kept_approximations_stay_inside_their_bound(torch, ctx, oracles, octx32, name, flavour, channel):
    ctx.set_fast(flavour == "float")
    ora = oracles[flavour]
    v = pdc.group_vectors(octx32.base, name)
    dic = pdc.Dictionary(octx32.base, octx32.det_rows, octx32.det[channel], flavour)
    group = [rp for rp, _ in pdc.replay_group(dic, v, ora, channel)]
    assert all(rp.r[0].dtype == pdc.dtype_of(flavour) for rp in group)
    want_p = [expected_values(torch, ctx, channel, rp) for rp in group]
    worst = 0.0
    for depth in pdc.DEPTHS:
        (counts, choices, _, swept), (P, meta, E) = run_stopped(ctx, channel, v, depth, FILLS[0])
        fill = FILLS[0]
        what = (name, flavour, channel, depth)
        # ---- records ----
        q = pdc.group_quant(v, depth)
        for i, rp in enumerate(group):
            cnt, d, k, _, S = ora.calc_mp(channel, v[i], quant=q)
            assert cnt == rp.end(depth) and counts[i] == cnt, (what, i, int(counts[i]), cnt)
            assert (choices["deltaId"][i, :cnt + 1] == d[:cnt + 1]).all() and (choices["intCoeff"][i, :cnt + 1] == k[:cnt + 1]).all(), (what, i)
            assert swept[i] == S, (what, i)
        # ---- bookkeeping: the one wave that ran the batch ----
        touched = [w for w in range(WAVES) if (u32(E[w]) != fill).any() or (meta[w] != fill).any() or (u32(P[w]) != fill).any()]
        assert len(touched) == 1 and touched[0] < 12, (what, touched)
        w = touched[0]
        for i, rp in enumerate(group):
            pairs = rp.pairs_at(depth)
            n, e = len(pairs), rp.end(depth)
            written = u32(E[w, i]) != fill
            assert written[:n].all() and not written[n:].any(), (what, i, n, written)
            assert [int(x) for x in meta[w, i, :n, 0]] == [p.meta() for p in pairs], (what, i)
            assert (meta[w, i, n:, 0] == fill).all() and (meta[w, i, :, 1] == fill).all(), (what, i)
            assert (u32(P[w, i, n:]) == fill).all(), (what, i)
            if n == 0:
                continue
            # ---- bound ----
            for p, pair in enumerate(pairs):
                model, u = pdc.bound_model(rp, pair, depth)
                assert abs(float(E[w, i, p]) - model) <= (u + 1) * 2.0 ** -22 * model, (what, i, p, u, float(E[w, i, p]), model)
            # ---- invariant ----
            got = P[w, i, :n]
            assert (u32(got[:, 62:]) == 0).all(), (what, i)                    # the pad rows
            exact = np.array([pdc.chain_dot(dic.block(pair.block), rp.r[e]) for pair in pairs]).astype(np.float64)
            ratio = np.abs(got[:, :62].astype(np.float64) - exact) / E[w, i, :n, None].astype(np.float64)
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (what, i, float(ratio.max()), np.argwhere(ratio > 1.0)[:4])
            # ---- values ----
            assert want_p[i][e].shape == got.shape, (what, i)
            same = u32(got) == u32(want_p[i][e])
            assert same.all(), (what, i, np.argwhere(~same)[:4], got[~same][:4], want_p[i][e][~same][:4])
        # ---- no stale reads: the other fill word ----
        (counts2, choices2, _, _), (P2, meta2, E2) = run_stopped(ctx, channel, v, depth, FILLS[1])
        assert (counts2 == counts).all() and (choices2 == choices).all(), what
        touched2 = [x for x in range(WAVES) if (u32(E2[x]) != FILLS[1]).any() or (meta2[x] != FILLS[1]).any()]
        assert len(touched2) == 1, (what, touched2)
        w2 = touched2[0]
        for i, rp in enumerate(group):
            n = len(rp.pairs_at(depth))
            assert (u32(P2[w2, i, :n]) == u32(P[w, i, :n])).all() and (u32(E2[w2, i, :n]) == u32(E[w, i, :n])).all(), (what, i)
            assert (meta2[w2, i, :n, 0] == meta[w, i, :n, 0]).all(), (what, i)
            assert (u32(P2[w2, i, n:]) == FILLS[1]).all() and (u32(E2[w2, i, n:]) == FILLS[1]).all(), (what, i)
            assert (meta2[w2, i, n:, 0] == FILLS[1]).all() and (meta2[w2, i, :, 1] == FILLS[1]).all(), (what, i)
        others = [x for x in range(WAVES) if x != w2]
        assert (u32(P2[others]) == FILLS[1]).all()
    print(f"pair drift, group {name}, {flavour}, channel {channel}: worst |P - exact| / E = {worst:.3g}")


def test_depth_1_is_the_probe_alone(torch, ctx, oracles, octx32):
    """at depth 1 the only pair of a slot has its MFMA start and no update: P and E are the probe's, bit for bit"""
    ctx.set_fast(False)
    v = pdc.group_vectors(octx32.base, "deep")
    dic = pdc.Dictionary(octx32.base, octx32.det_rows, octx32.det[0], "double")
    group = [rp for rp, _ in pdc.replay_group(dic, v, oracles["double"], 0)]
    _, (P, meta, E) = run_stopped(ctx, 0, v, 1, FILLS[0])
    w, = [x for x in range(WAVES) if (u32(E[x]) != FILLS[0]).any()]
    for i, rp in enumerate(group):
        pair, = rp.pairs_at(1)
        assert pair.created == 0 and pair.first == pdc.NUM_BASE
        start, bound = mfma_start(torch, ctx, 0, pair.block, rp.r[1])
        assert (u32(P[w, i, 0]) == u32(start)).all() and u32(E[w, i, 0]) == u32(np.float32(bound)), i


def test_refusals(ia, torch, ctx):
    A = ia.api.MPC_ERR_ARGUMENT
    L = ia.load_library()
    total = 16 * torch.cuda.get_device_properties(0).multi_processor_count       # one workgroup per compute unit, 16 scratch waves each
    SENT = 0x5EA1
    per = 16 * 32
    hp = np.full(2 * per * 64, SENT, np.uint32)
    hm = np.full(2 * per * 2, SENT, np.uint32)
    he = np.full(2 * per, SENT, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(begin, count, fill=1, word=0xDEADBEEF, p=hp, m=hm, e=he, h=ctx.h):
        return L.mpc_debug_pair_scratch(h, begin, count, fill, word, ptr(p) if p is not None else None,
                                        ptr(m) if m is not None else None, ptr(e) if e is not None else None)
    mark = 0x12345678
    ctx.debug_pair_scratch(0, 2, mark)
    ctx.debug_pair_scratch(total - 1, 1, mark)
    for begin, count in ((-1, 1), (0, 0), (0, -1), (total, 1), (total - 1, 2), (0, total + 1), (1, total), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1),
                         (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, 2)):
        assert call(begin, count) == A, (begin, count)
    for fill in (2, -1):
        assert call(0, 1, fill=fill) == A
    assert call(0, 1, p=None) == A and call(0, 1, m=None) == A and call(0, 1, e=None) == A
    assert call(0, 1, h=None) == A
    host = ia.create_compression_context(8, 8, 3.5, device=-1)
    assert call(0, 1, h=host.h) == ia.api.MPC_ERR_NO_DEVICE
    host.close()
    # nothing was written: neither the host buffers nor the scratch
    assert (hp == SENT).all() and (hm == SENT).all() and (he == SENT).all()
    for begin, count in ((0, 2), (total - 1, 1)):                       # ... and the last valid wave is accepted
        assert all((u32(a) == mark).all() for a in ctx.debug_pair_scratch(begin, count))
    # fill = 0 writes nothing either, whatever the word
    assert call(0, 2, fill=0, word=0xDEADBEEF) == ia.api.MPC_OK
    assert (hp == mark).all() and (hm == mark).all() and (he == mark).all()
    assert all((u32(a) == mark).all() for a in ctx.debug_pair_scratch(0, 2))
