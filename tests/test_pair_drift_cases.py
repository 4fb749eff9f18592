"""The inputs and host models of test_gpu_pair_drift.py do what they claim -- shown from the oracle alone (no GPU).

The host replay of the pursuit (tests/pair_drift_cases.py) is held to the oracle for every group, flavour, channel, vector and
stop depth: same counts and indices, the low 16 bits of the zig-zag of its q are the oracle's intCoeff, and its residual at the
stop is the oracle's bit for bit.  From the replays the test then asserts that the groups put the kept approximations through what
the device test is there for (many updates of one pair, the meta route, more than one round of items, ended slots beside live
ones, atoms inside and outside the updated pair's block, a repeated base row, rows of DetailBasis[0]); a group that misses its
condition fails.  The float fused multiply-add of the expected values is held to rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import pair_drift_cases as pdc
import pair_round_cases as prc


@pytest.fixture(scope="module")
def oracles(oracle, octx32):
    return {"double": octx32, "float": oracle.OracleFastContext(octx32)}


@pytest.fixture(scope="module")
def replays(oracles, octx32):
    """(group, flavour, channel) -> (vectors, dictionary, [(replay, oracle result at the deepest stop)])"""
    out = {}
    for flavour in pdc.FLAVOURS:
        for ch in pdc.CHANNELS:
            dic = pdc.Dictionary(octx32.base, octx32.det_rows, octx32.det[ch], flavour)
            for name in pdc.GROUPS:
                v = pdc.group_vectors(octx32.base, name)
                out[(name, flavour, ch)] = (v, dic, pdc.replay_group(dic, v, oracles[flavour], ch))
    return out


def bits(a, flavour):
    return np.ascontiguousarray(a, pdc.dtype_of(flavour)).view(np.uint64 if flavour == "double" else np.uint32)


def test_groups_and_depths():
    assert all(0 < d < pdc.K for d in pdc.DEPTHS) and pdc.DEPTHS == (1, 2, 3, 5, 9, 17, 24, 31)
    assert set(pdc.GROUPS) >= {"ramp", "deep", "mixed", "one"} and all(len(prc.GROUPS[g]) == 16 for g in ("ramp", "deep", "mixed", "one"))


def test_scaled_groups_are_exact_scalings(octx32):
    deep = pdc.group_vectors(octx32.base, "deep")
    for name, s in pdc.SCALED.items():
        v = pdc.group_vectors(octx32.base, name)
        assert (v == deep * s).all() and (v.astype(np.float32).astype(np.float64) == v).all()
        assert (pdc.group_quant(v, 5)[:5] == pdc.group_quant(deep, 5)[:5] * s).all() and pdc.group_quant(v, 5)[5] == pdc.STOP


def test_group_with_row_0_holds_row_0(octx32):
    v = pdc.group_vectors(octx32.base, "with_row0")
    want = 900.0 * pdc.ROW0_DECAY ** (1 + np.arange(16) % 3)           # the other base rows sum to zero: row 0's weight is its projection
    assert v.shape == (16, 64) and np.allclose(v @ octx32.base[0], want, rtol=1e-6, atol=0)
    assert (v.astype(np.float32).astype(np.float64) == v).all()


def test_every_pair_block_has_62_rows(octx32):
    rows = octx32.det_rows
    assert [b for b in range(pdc.NUM_BASE) if rows[b] != 62] == [0, 509] and rows[0] == rows[509] == 63
    assert (octx32.base[509] == -octx32.base[0]).all()                # loses the tie to row 0: block 509 is never unlocked


@pytest.mark.parametrize("channel", pdc.CHANNELS)
@pytest.mark.parametrize("flavour", pdc.FLAVOURS)
@pytest.mark.parametrize("name", pdc.GROUPS)
def test_replay_is_the_oracle_s_pursuit_at_every_depth(replays, oracles, name, flavour, channel):
    v, dic, group = replays[(name, flavour, channel)]
    ora = oracles[flavour]
    for i, (rp, full) in enumerate(group):
        assert all(p.rows == 62 and 0 < p.block < 509 for p in rp.pairs)
        for depth in pdc.DEPTHS:
            what = (name, flavour, channel, i, depth)
            q = pdc.group_quant(v, depth)
            cnt, d, k, res, _ = ora.calc_mp(channel, v[i], quant=q) if depth != pdc.DEPTHS[-1] else full
            e = rp.end(depth)
            assert cnt == e, what                                               # the steps before the stop do not depend on it
            assert prc.chosen_ids(cnt, d) == rp.ids[:e], what
            assert [pdc.zigzag(rp.q[s]) & 0xFFFF for s in range(e)] == [int(x) for x in k[:e]], what
            assert (bits(res, flavour) == bits(rp.r[e], flavour)).all(), what   # the oracle's residual is r_e
            end_id = prc.chosen_ids(cnt + 1, d)[-1]
            assert k[cnt] == 0 and rp.ending_q(dic, q, end_id, e) == 0, what    # the ending step quantises to 0
        # the intCoeff record alone would not give q back
        assert name == "one" or any(pdc.zigzag(x) > 0xFFFF for x in rp.q) or rp.count == 0, (name, i)


@pytest.mark.parametrize("channel", pdc.CHANNELS)
@pytest.mark.parametrize("flavour", pdc.FLAVOURS)
def test_groups_meet_their_conditions(replays, flavour, channel):
    deepest = pdc.DEPTHS[-1]
    old = [rp for name in ("ramp", "deep", "mixed") for rp, _ in replays[(name, flavour, channel)][2]]
    updates = max(len(rp.updates(p, deepest)) for rp in old for p in rp.pairs)
    assert updates >= 24, updates                                               # one pair is updated 24 times or more
    every = [rp for name in pdc.GROUPS for rp, _ in replays[(name, flavour, channel)][2]]
    assert max(len(rp.pairs) for rp in old) > 4 and max(len(rp.pairs) for rp in every) > 8      # the pair_meta route (p >= 4), well into it
    assert all(len(rp.pairs) < pdc.MAX_PAIRS for rp in every)
    own = other = zero_block = 0
    for rp in old:
        for s in range(rp.count):
            held = [p for p in rp.pairs if p.created < s]
            if rp.atom_block[s] > 0:                                            # a detail row of a pair's block, chosen while pairs are held
                own += sum(1 for p in held if p.block == rp.atom_block[s])
                other += sum(1 for p in held if p.block != rp.atom_block[s])
    assert own >= 100 and other >= 100, (own, other)
    assert any(rp.repeats for rp in old)                                        # a repeated base row: rows appended, no pair
    for name in pdc.GROUPS:
        group = [rp for rp, _ in replays[(name, flavour, channel)][2]]
        if name in ("ramp", "deep", "mixed", "with_row0") + tuple(pdc.SCALED):
            assert max(sum(rp.items(s, deepest) for rp in group) for s in range(pdc.K)) > 16, name      # more than one round
    # a stop depth that leaves slots which ended earlier beside slots that went on to it
    mixed = [rp for rp, _ in replays[("mixed", flavour, channel)][2]]
    assert any(any(rp.count < d for rp in mixed) and any(rp.count >= d and rp.pairs_at(d) for rp in mixed) for d in pdc.DEPTHS)
    ramp = [rp for rp, _ in replays[("ramp", flavour, channel)][2]]
    assert any(0 < rp.count < 3 for rp in ramp) and any(rp.count == deepest for rp in ramp)
    # rows of DetailBasis[0] chosen while pairs are held
    for rp, _ in replays[("with_row0", flavour, channel)][2]:
        for s in range(rp.count):
            if rp.atom_block[s] == 0:
                assert rp.unlock0 is not None and rp.unlock0 < s
                zero_block += sum(1 for p in rp.pairs if p.created < s)
    assert zero_block >= 10, zero_block
    # the scaled groups are the same pursuit: same indices, same q
    deep = replays[("deep", flavour, channel)][2]
    for name in pdc.SCALED:
        for (a, _), (b, _) in zip(deep, replays[(name, flavour, channel)][2]):
            assert a.ids == b.ids and a.q == b.q, name


def test_bound_model_grows_by_the_recurrence(replays):
    _, _, group = replays[("deep", "float", 0)]
    rp = group[0][0]
    pair = rp.pairs[0]
    E0, u0 = pdc.bound_model(rp, pair, pair.created + 1)
    assert u0 == 0 and abs(E0 - 2.0 ** -13 * pdc.rnorm_model(rp.r[pair.created + 1])) <= 2.0 ** -22 * E0
    E, u = pdc.bound_model(rp, pair, pdc.DEPTHS[-1])
    assert u == rp.end(pdc.DEPTHS[-1]) - pair.created - 1 and u >= 24 and E > E0
    j = pair.created + 1
    E1, u1 = pdc.bound_model(rp, pair, j + 1)
    assert u1 == 1 and E1 == (E0 + 2.0 ** -21 * (abs(float(np.float32(rp.c[j]))) + pdc.rnorm_model(rp.r[j]))) * pdc.GROW


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(5)
    b = rng.standard_normal(4096).astype(np.float32)
    c = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-6, 3, 4096)).astype(np.float32)
    a = np.float32(-1234.567)
    got = pdc.fma32(a, b, c)
    for k in range(0, 4096, 7):
        want = pdc._nearest_f32(Fraction(float(a)) * Fraction(float(b[k])) + Fraction(float(c[k])))
        assert got[k].view(np.uint32) == want.view(np.uint32), k
    H = 2.0 ** -24                                                     # half a float32 step at 1
    # exact ties go to the even significand
    tie = pdc.fma32(np.float32(1.0), np.array([H, H], np.float32), np.array([1.0, 1.0 + 2 * H], np.float32))
    assert tie.tolist() == [1.0, 1.0 + 4 * H]
    # the float64 sum is a tie, the exact sum is not: a * b = +-H (1 - 2^-46), and H 2^-46 is lost beside c in float64
    a = np.float32(1.0 + 2 * H)
    b = np.array([H * (1.0 - 2 * H), -H * (1.0 - 2 * H)], np.float32)
    c = np.array([1.0 + 2 * H, 1.0 + 2 * H], np.float32)
    assert (b.astype(np.float64) == np.array([H * (1.0 - 2 * H), -H * (1.0 - 2 * H)])).all()
    assert (np.float64(a) * b.astype(np.float64) + c.astype(np.float64) == np.array([1.0 + 3 * H, 1.0 + H])).all()
    assert pdc.fma32(a, b, c).tolist() == [1.0 + 2 * H, 1.0 + 2 * H]   # rounding the float64 sum would give 1 + 4 H and 1


def test_scratch_entry_refuses_without_a_device():
    """mpc_debug_pair_scratch checks its arguments before it touches anything: no context, and a context without a device"""
    import ctypes as C

    import imageexperiments_amd as ia
    L = ia.load_library()
    bufs = [np.full(16 * 32 * n, 7, np.uint32) for n in (64, 2, 1)]
    ptrs = [b.ctypes.data_as(C.c_void_p) for b in bufs]
    assert L.mpc_debug_pair_scratch(None, 0, 1, 1, 0, *ptrs) == ia.api.MPC_ERR_ARGUMENT
    host = ia.create_compression_context(8, 8, 3.5, device=-1)
    assert L.mpc_debug_pair_scratch(host.h, 0, 1, 1, 0, *ptrs) == ia.api.MPC_ERR_NO_DEVICE
    with pytest.raises(ia.MpcError) as e:
        host.debug_pair_scratch(0, 1)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host.close()
    assert all((b == 7).all() for b in bufs)
