"""The pair rounds of the pursuit kernel (run with -m gpu): groups of 16 vectors -- one wave's slots -- whose pair updates fill
the rounds of 16 items partly, exactly, several times over and across round boundaries (tests/pair_round_cases.py;
tests/test_pair_round_cases.py shows on the CPU that they do).  Both flavours, channels 0 and 2, bit equality with the oracle's
calc_mp: counts, records 0..count inclusive, swept rows and the bits of the residual energy."""
import numpy as np
import pytest

import pair_round_cases as prc
import pursuit_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def contexts(ia, oracle, octx32):
    double = ia.create_compression_context(prc.K, 8, 3.5, device=0)
    fast = ia.create_compression_context(prc.K, 8, 3.5, device=0).set_fast(True)
    yield {"double": (double, octx32), "float": (fast, oracle.OracleFastContext(octx32))}
    double.close()
    fast.close()


def _energy64(res):
    e = 0.0                                                   # sum of squares in element order, every step rounded to double
    for x in np.asarray(res, np.float64):
        e = e + x * x
    return e


@pytest.mark.parametrize("channel", [0, 2])
@pytest.mark.parametrize("flavour", ["double", "float"])
@pytest.mark.parametrize("name", list(prc.GROUPS))
def test_group_is_bit_identical_to_the_oracle(contexts, octx32, name, flavour, channel):
    ctx, ora = contexts[flavour]
    v = prc.group_vectors(octx32.base, name)
    q = prc.group_quant(v)
    counts, choices, energy, swept = ctx.calc_mp(channel, v, quant_k=q)      # one call: 16 consecutive vectors share a wave
    for i in range(v.shape[0]):
        cnt, d, k, res, S = ora.calc_mp(channel, v[i], quant=q)
        what = (name, flavour, channel, i)
        assert counts[i] == cnt, (what, int(counts[i]), cnt)
        n = min(cnt + 1, prc.K)                                              # records 0..count inclusive
        assert (choices["deltaId"][i, :n] == d[:n]).all(), what
        assert (choices["intCoeff"][i, :n] == k[:n]).all(), what
        assert swept[i] == S, what
        want = _energy64(res) if flavour == "double" else pc.f32_energy(res)
        assert np.float64(energy[i]).view(np.uint64) == np.float64(want).view(np.uint64), (what, energy[i], want)
