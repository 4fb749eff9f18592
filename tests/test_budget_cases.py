"""The rate control on the host: mpc_budget_allocate, mpc_budget_weights and mpc_budget_lambda against the numpy model of
tests/budget_cases.py on every case, the cases against the mistakes they are there to catch, refusals.  No GPU."""
import numpy as np
import pytest

import budget_cases as bc

CASES = bc.cases()


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def test_lambda_is_the_table(ia):
    table = [ia.budget_lambda(j) for j in range(bc.LAMBDAS)]
    assert table == [bc.lambda_of(j) for j in range(bc.LAMBDAS)]
    assert table[:10] == [0, 8, 9, 10, 11, 12, 13, 14, 15, 16] and table[255] == 14 << 31 and ia.api.MPC_BUDGET_LAMBDAS == 256
    assert all(b > a for a, b in zip(table, table[1:]))
    # a geometric grid in steps of about 10 %: between 1/15 and 1/8 from j = 1 on
    assert all(1 / 15 <= (b - a) / a <= 1 / 8 for a, b in zip(table[1:], table[2:]))
    # one bit of a record at j = 255 costs more than a tile's largest possible distortion term
    assert table[255] * bc.W_MIN > bc.P_MAX * 65536 and table[255] * (3 * 32 * bc.W_MAX) + bc.P_MAX * 65536 < 1 << 64
    for j in (-1, 256, 1 << 20):
        with pytest.raises(ia.MpcError) as e:
            ia.budget_lambda(j)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_allocate_is_the_model(ia, case):
    name, P, counts, W, js = case
    for j in js:
        depth, cut, totals = ia.budget_allocate(P, counts, W, j)
        want_depth, want_cut, want_totals = bc.allocate(P, counts, W, j)
        assert depth.dtype == np.uint8 and (depth == want_depth).all(), (name, j)
        assert cut.dtype == np.uint16 and (cut == want_cut).all(), (name, j)
        assert [int(v) for v in totals] == want_totals, (name, j)
        if j == 255:
            assert not depth.any() and not cut.any() and totals[1] == 0 and totals[2] == 0
            assert int(totals[0]) == int(P[:, 0].astype(np.int64).sum())


def test_the_cases_cover_what_the_contract_names():
    names = [c[0] for c in CASES]
    for K in (1, 32):
        for T in (1, 63, 64, 65):
            assert f"K{K} T{T} monotone" in names and f"K{K} T{T} not monotone" in names
    assert "K8 T4097" in names
    for name, P, counts, W, js in CASES:
        assert P.dtype == np.uint32 and counts.dtype == np.uint16 and W.dtype == np.uint32
        assert P.shape == (counts.shape[0], W.shape[1] + 1) and int(P.max()) <= bc.P_MAX
        assert int(W.min()) >= bc.W_MIN and int(W.max()) <= bc.W_MAX
        if "not monotone" in name and P.shape[1] > 2 and P.shape[0] > 1:
            assert (np.diff(P.astype(np.int64), axis=1) > 0).any(), name
        if name.startswith("K32 T65"):
            assert (counts == 0).all(axis=1).any() and (counts[:, 0] != counts[:, 1]).any()
    assert {0, 255} <= set(CASES[0][4])
    # the ties are ties: every depth of "exact ties" has the same J at its first multiplier
    name, P, counts, W, js = next(c for c in CASES if c[0] == "K8 exact ties")
    R = bc.rates(counts, W, 8)
    assert len({int(P[0, n]) * 65536 + bc.lambda_of(js[0]) * R[0, n] for n in range(9)}) == 1


@pytest.mark.parametrize("mistake", bc.WRONG)
def test_the_cases_tell_the_model_from_a_wrong_allocation(mistake):
    caught = []
    for name, P, counts, W, js in CASES:
        for j in js:
            want, got = bc.allocate(P, counts, W, j), bc.allocate(P, counts, W, j, mistake)
            if (want[0] != got[0]).any() or (want[1] != got[1]).any() or want[2] != got[2]:
                caught.append((name, j))
    assert caught, mistake


def test_allocate_refusals(ia):
    L = ia.load_library()
    P, c, W, t = np.zeros(9, np.uint32), np.zeros(3, np.uint16), np.full(24, 256, np.uint32), np.zeros(3, np.uint64)
    u32, u16, u64 = ia.api._u32p, ia.api._u16p, ia.api.C.POINTER(ia.api.C.c_uint64)
    ok = lambda tiles, K, j: L.mpc_budget_allocate(P.ctypes.data_as(u32), c.ctypes.data_as(u16), tiles, K, W.ctypes.data_as(u32), j, None, None,
                                                   t.ctypes.data_as(u64))
    assert ok(1, 8, 3) == ia.api.MPC_OK and ok(0, 8, 3) == ia.api.MPC_OK         # depth and out_counts may be null; no tiles is no work
    for tiles, K, j in ((-1, 8, 0), (1, 0, 0), (1, 33, 0), (1, 8, -1), (1, 8, 256)):
        assert ok(tiles, K, j) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_budget_allocate(None, c.ctypes.data_as(u16), 1, 8, W.ctypes.data_as(u32), 0, None, None, t.ctypes.data_as(u64)) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_budget_allocate(P.ctypes.data_as(u32), c.ctypes.data_as(u16), 1, 8, W.ctypes.data_as(u32), 0, None, None, None) == ia.api.MPC_ERR_ARGUMENT


def test_weights_of_the_golden_container(ia, mn_bytes):
    _, _, K, _ = ia.container_info(mn_bytes)
    for interval, expanded in ((0, 0), (32, 1), (4096, 1)):                         # either version, any interval: the same weights
        index = ia.container_index2(mn_bytes, interval, expanded)
        streams = ia.index_info(index)["streams"]
        W = ia.budget_weights(index)
        assert W.dtype == np.uint32 and W.shape == (3, K) and (W == bc.weights_from_streams(streams, K)).all()
        assert int(W.min()) >= bc.W_MIN and int(W.max()) <= bc.W_MAX
    # the first luma steps of a photograph cost several bits a record; a step no tile reaches costs the floor
    assert W[0, 0] > 2 * bc.W_MIN and (W[0, :4] > bc.W_MIN).all()
    empty = [(ch, i) for ch in range(3) for i in range(K) if streams[1 + 2 * K * ch + 2 * i]["expect"] == 0]
    assert all(W[ch, i] == bc.W_MIN for ch, i in empty)


def test_weights_are_clamped(ia):
    """4096 tiles that all hold the same single record: the run-length coded streams take far less than a bit a record, and a
    stream of one record under its wrapper far more than a few bits: the floor holds, and the model without the clamp differs."""
    K, T = 2, 4096
    counts = np.zeros((T, 3), np.uint16)
    counts[:, 0] = 1
    counts[0, 1] = 2
    choices = np.zeros((T, 3, K), np.uint32)
    choices[:, 0, 0] = 5 | (7 << 16)
    choices[0, 1] = (300 | (40000 << 16), 17 | (3 << 16))
    blob = ia.assemble_streams(512, 512, K, 8, np.ones((3, K)), counts.reshape(-1), choices)
    index = ia.container_index(blob)
    streams = ia.index_info(index)["streams"]
    W, loose = ia.budget_weights(index), bc.weights_from_streams(streams, K, clamp=False)
    assert (W == bc.weights_from_streams(streams, K)).all()
    assert W[0, 0] == bc.W_MIN and loose[0, 0] < bc.W_MIN                          # 4096 records in a handful of bits
    assert W[1, 1] > 16 * bc.W_MIN                                                 # one record and two wrappers
    assert (np.array(loose, np.int64) != W.astype(np.int64)).any()


def _weights_status(ia, blob):
    """mpc_budget_weights as it is, into room for any K -> status"""
    W = np.zeros((3, 32), np.uint32)
    buf = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    return ia.load_library().mpc_budget_weights(buf.ctypes.data_as(ia.api._u8p), len(blob), W.ctypes.data_as(ia.api._u32p))


def test_weights_refusals(ia, mn_bytes):
    index = ia.container_index(mn_bytes)
    assert _weights_status(ia, index) == ia.api.MPC_OK
    refused = 0
    for label, blob in bc.damaged_indexes(index):
        try:
            ia.index_info(blob)
            readable = True
        except ia.MpcError as e:
            assert e.status == ia.api.MPC_ERR_BITSTREAM
            readable = False
        st = _weights_status(ia, blob)
        if not readable:                                                           # what mpc_index_info refuses
            assert st == ia.api.MPC_ERR_BITSTREAM, label
            refused += 1
        else:                                                                      # a flipped bit in a size: other weights, or a refusal
            assert st in (ia.api.MPC_OK, ia.api.MPC_ERR_BITSTREAM, ia.api.MPC_ERR_ARGUMENT), label
    assert refused >= 6
    serial = bytearray(index)                                                      # the header's flag word: "serial only"
    serial[12] |= 1
    assert ia.index_info(bytes(serial))["serial_only"] and _weights_status(ia, bytes(serial)) == ia.api.MPC_ERR_ARGUMENT
    L = ia.load_library()
    W = np.zeros((3, 32), np.uint32)
    buf = np.frombuffer(index, np.uint8)
    assert L.mpc_budget_weights(None, buf.size, W.ctypes.data_as(ia.api._u32p)) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_budget_weights(buf.ctypes.data_as(ia.api._u8p), buf.size, None) == ia.api.MPC_ERR_ARGUMENT
