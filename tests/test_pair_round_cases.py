"""The inputs of test_gpu_pair_rounds.py do what they claim -- shown from the oracle alone (no GPU).

The device updates a wave's pairs in rounds of 16 items (tests/pair_round_cases.py).  From the oracle's records of every group
this test reconstructs each vector's chosen dictionary indices, hence the blocks it unlocked and its number of pairs at every
step, and asserts that the groups put the rounds through every case that matters; a group that misses its condition fails."""
import pytest

import pair_round_cases as prc

FLAVOURS = ("double", "float")
CHANNELS = (0, 2)


@pytest.fixture(scope="module")
def waves(oracle, octx32):
    """(group, flavour, channel) -> one analysis per wave of 16 vectors"""
    ofast = oracle.OracleFastContext(octx32)
    out = {}
    for name in prc.GROUPS:
        v = prc.group_vectors(octx32.base, name)
        q = prc.group_quant(v)
        for flavour in FLAVOURS:
            o = octx32 if flavour == "double" else ofast
            for ch in CHANNELS:
                res = [o.calc_mp(ch, v[i], quant=q) for i in range(v.shape[0])]
                out[(name, flavour, ch)] = [prc.analyse([r[0] for r in res[w:w + 16]], [r[1] for r in res[w:w + 16]])
                                            for w in range(0, len(res), 16)]
    return out


def test_groups_are_whole_waves():
    for name, rows in prc.GROUPS.items():
        assert len(rows) % 16 == 0 and len(rows) > 0, name
    assert len(prc.GROUPS["ramp_reversed_4_waves"]) == 64
    assert prc.GROUPS["ramp_reversed_4_waves"][:16] == prc.RAMP[::-1]


@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_group_meets_its_condition(waves, flavour, channel):
    ramp, = waves[("ramp", flavour, channel)]
    assert any(1 <= t <= 15 for t in ramp["totals"]), ramp["totals"]              # a round that is not full
    assert any(t > 64 for t in ramp["totals"]), ramp["totals"]                    # more than four rounds
    assert any(t > 16 and t % 16 for t in ramp["totals"]), ramp["totals"]
    assert ramp["max_pairs"] > 4                                                  # pair_meta instead of the packed words
    assert ramp["ends_early"] and sum(1 for c in ramp["counts"] if c <= 2) == 2   # two slots end at once, the others go on
    deep, = waves[("deep", flavour, channel)]
    assert deep["totals"][1] == 16, deep["totals"]                                # exactly one full round
    assert any(t > 64 for t in deep["totals"]) and all(c == prc.K for c in deep["counts"])
    assert all(a <= b for a, b in zip(deep["totals"][:-1], deep["totals"][1:-1]))
    mixed, = waves[("mixed", flavour, channel)]
    early = sum(1 for c in mixed["counts"] if c <= 2)
    assert early >= 6 and sum(1 for c in mixed["counts"] if c == prc.K) == 16 - early, mixed["counts"]
    assert mixed["ends_early"] and 16 in mixed["totals"]
    one, = waves[("one", flavour, channel)]
    assert one["fresh_only"] and one["max_pairs"] == 1
    if flavour == "double":                                                       # one fresh pair and no update at all
        assert all(c == 1 for c in one["counts"]) and sum(one["totals"]) == 0, one


def test_the_cases_between_them_cover_the_rounds(waves):
    every = [a for w in waves.values() for a in w]
    totals = [t for a in every for t in a["totals"]]
    assert any(1 <= t <= 15 for t in totals)
    assert 16 in totals
    assert any(t > 16 and t % 16 for t in totals)
    assert any(t > 64 for t in totals)
    assert any(a["max_pairs"] > 4 for a in every) and any(a["max_pairs"] > 8 for a in every)
    assert any(a["ends_early"] for a in every)
    assert any(a["fresh_only"] for a in every)
    # the four waves of the reversed ramp do not repeat the ramp's totals: their levels meet the round boundaries elsewhere
    for flavour in FLAVOURS:
        for ch in CHANNELS:
            ramp, = waves[("ramp", flavour, ch)]
            assert all(a["totals"] != ramp["totals"] for a in waves[("ramp_reversed_4_waves", flavour, ch)])
