"""The pursuit kernel's key tracking on the device (run with -m gpu): mpc_debug_track_probe_device runs the kernel's own track_tile and
pair_keys (mp_pursuit.hip) in one wave on given bit patterns, by the definition (four TopKeys::see) and grouped (TopKeys::see4), laid
out as pass 1 and the pair rounds see them: 36 tiles x 4 values per lane with the row codes, 16 values of a pair per lane with the pair
codes, the pad rule of 62-, 63- and 64-row blocks and the largest |P|.

Three-way equality, bit for bit: device by the definition == device grouped == the numpy model (tests/track_keys_cases.py; the
case classes are those of tests/test_track_keys_model.py).  NaN and infinity are out of scope, see there."""
import numpy as np
import pytest

import track_keys_cases as tk

pytestmark = pytest.mark.gpu

CASES = tk.device_cases()
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    import imageexperiments_amd as ia
    c = ia.create_compression_context(8, 8, 3.5, device=0)
    yield c
    c.close()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_definition_grouped_and_model_agree(torch, ctx, case):
    name, row_bits, pair_bits, bound, rows, pair = case
    d_rows, d_pairs = dev(torch, row_bits), dev(torch, pair_bits)
    out = dev(torch, np.full((tk.LANES, 14), SENTINEL, np.uint32))
    ctx.debug_track_probe_device(d_rows.data_ptr(), d_pairs.data_ptr(), bound, rows, pair, out.data_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    model = tk.track_rows(row_bits, tk.see4_sequential)
    mp = tk.track_pair(pair_bits, bound, rows, pair, tk.see4_sequential)
    seq = [o[:, 0], o[:, 1], o[:, 4], o[:, 5]]
    grp = [o[:, 2], o[:, 3], o[:, 6], o[:, 7]]
    for what, s, g, m in zip(("base k1", "base k2", "block k1", "block k2"), seq, grp, model):
        assert np.array_equal(s, g), (name, what, "definition != grouped")
        assert np.array_equal(s, m), (name, what, "device != model")
    for what, s, g, m in zip(("pair k1", "pair k2", "largest |P|"), o[:, 8:11].T, o[:, 11:14].T, mp):
        assert np.array_equal(s, g), (name, what, "definition != grouped")
        assert np.array_equal(s, m), (name, what, "device != model")


def test_arguments_are_checked(torch, ctx):
    import imageexperiments_amd as ia
    p = dev(torch, np.zeros((tk.LANES, tk.ROW_VALUES), np.uint32)).data_ptr()

    def refused(call):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT

    refused(lambda: ctx.debug_track_probe_device(0, p, 0.0, 64, 0, p))
    refused(lambda: ctx.debug_track_probe_device(p, 0, 0.0, 64, 0, p))
    refused(lambda: ctx.debug_track_probe_device(p, p, 0.0, 64, 0, 0))
    refused(lambda: ctx.debug_track_probe_device(p + 4, p, 0.0, 64, 0, p))
    refused(lambda: ctx.debug_track_probe_device(p, p + 8, 0.0, 64, 0, p))
    for rows in (0, 65):
        refused(lambda: ctx.debug_track_probe_device(p, p, 0.0, rows, 0, p))
    for pair in (-1, 32):
        refused(lambda: ctx.debug_track_probe_device(p, p, 0.0, 64, pair, p))
    host = ia.create_compression_context(8, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        host.debug_track_probe_device(p, p, 0.0, 64, 0, p)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host.close()
