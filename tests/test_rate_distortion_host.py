"""Rate-distortion sweep, host side (no GPU): mpc_quant_tables against the oracle and a host-only context, the header values of
the reference's own container, argument errors of the three new entry points and the Python parsing of quality levels."""
import ctypes as C

import numpy as np
import pytest

BPPS = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 3.5, 12.0]


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.mark.parametrize("K", [1, 8, 16, 32])
def test_quant_tables_equal_the_oracle_and_a_host_context(ia, oracle, K):
    L = oracle.lib()
    dp = C.POINTER(C.c_double)
    for bpp in BPPS:
        q = ia.quant_tables(K, bpp)
        o = np.zeros((3, K))
        L.mpo_quant_tables(K, 8, bpp, o[0].ctypes.data_as(dp), o[1].ctypes.data_as(dp), o[2].ctypes.data_as(dp))
        assert np.array_equal(q, o), (K, bpp)
        ctx = ia.create_compression_context(K, 8, bpp, device=-1)
        assert np.array_equal(q, ctx.quant), (K, bpp)
        ctx.close()


def test_quant_tables_reproduce_the_reference_container_header(ia, mn_bytes):
    s = ia.read_compressed(mn_bytes)
    assert s["K"] == 32
    header = np.asarray(s["quant"], np.float64).reshape(3, 32)
    assert np.array_equal(ia.quant_tables(32, 3.5), header)


def test_quant_tables_argument_errors(ia):
    L = ia.load_library()
    q = np.zeros(3 * 33)
    dp = q.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mpc_quant_tables(0, 8, 3.5, dp) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_quant_tables(33, 8, 3.5, dp) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_quant_tables(8, 9, 3.5, dp) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_quant_tables(8, 8, float("inf"), dp) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_quant_tables(8, 8, float("nan"), dp) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_quant_tables(8, 8, 3.5, None) == ia.api.MPC_ERR_ARGUMENT


def test_new_entry_points_refuse_a_host_only_context(ia):
    L = ia.load_library()
    ctx = ia.create_compression_context(8, 8, 3.5, device=-1)
    rgb = np.zeros((8, 8, 3), np.uint8)
    quants = np.ones((2, 3, 8))
    sizes = (C.c_size_t * 2)()
    qp = quants.ctypes.data_as(C.POINTER(C.c_double))
    fake = C.c_void_p(rgb.ctypes.data)               # never dereferenced: the context is refused first
    for fn in (L.mpc_rate_distortion, L.mpc_rate_distortion_device):
        assert fn(ctx.h, fake, 8, 8, qp, 2, sizes, None, None, None) == ia.api.MPC_ERR_NO_DEVICE
        # bad arguments are reported as such on any context
        assert fn(ctx.h, fake, 8, 8, qp, 0, sizes, None, None, None) == ia.api.MPC_ERR_ARGUMENT
        assert fn(ctx.h, fake, 8, 8, None, 2, sizes, None, None, None) == ia.api.MPC_ERR_ARGUMENT
        assert fn(ctx.h, fake, 0, 8, qp, 2, sizes, None, None, None) == ia.api.MPC_ERR_ARGUMENT
        assert fn(ctx.h, fake, 8, -1, qp, 2, sizes, None, None, None) == ia.api.MPC_ERR_ARGUMENT
        assert fn(ctx.h, None, 8, 8, qp, 2, sizes, None, None, None) == ia.api.MPC_ERR_ARGUMENT
        assert fn(ctx.h, fake, 8, 8, qp, 2, None, None, None, None) == ia.api.MPC_ERR_ARGUMENT
        assert fn(None, fake, 8, 8, qp, 2, sizes, None, None, None) == ia.api.MPC_ERR_ARGUMENT
    sse = C.c_ulonglong(0)
    assert L.mpc_distortion_device(ctx.h, fake, fake, None, fake, 8, 8, C.byref(sse), None, None) == ia.api.MPC_ERR_NO_DEVICE
    assert L.mpc_distortion_device(ctx.h, fake, fake, None, fake, 8, 8, None, None, None) == ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_distortion_device(None, fake, fake, None, fake, 8, 8, C.byref(sse), None, None) == ia.api.MPC_ERR_ARGUMENT
    with pytest.raises(ia.MpcError) as e:
        ctx.rate_distortion(rgb, [3.5, "max"])
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    ctx.close()


def test_quality_parsing(ia):
    K = 8
    labels, q = ia.parse_qualities("max", K)
    assert labels == ["max"] and q.shape == (1, 3, K) and (q == 1.0).all()
    labels, q = ia.parse_qualities(3.5, K)
    assert labels == [3.5] and np.array_equal(q[0], ia.quant_tables(K, 3.5))
    table = np.arange(3 * K, dtype=np.float64).reshape(3, K) + 0.5
    labels, q = ia.parse_qualities([8, 1.0, "max", table], K)
    assert labels == [8.0, 1.0, "max", "table"]
    assert q.shape == (4, 3, K) and q.dtype == np.float64 and q.flags.c_contiguous
    assert np.array_equal(q[0], ia.quant_tables(K, 8.0))
    assert np.array_equal(q[3], table)
    labels, q = ia.parse_qualities(table, K)                 # one bare table is one level
    assert labels == ["table"] and np.array_equal(q[0], table)
    for bad in (["min"], [np.ones((3, K + 1))], [np.ones(3 * K)], [], [float("nan")], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            ia.parse_qualities(bad, K)
