"""The host half of the sequence decoder (no GPU): the container's header alone, and the serial half of readCompressed on its
own -- the streams as entropy-decoded, still run-length packed and difference coded -- against the whole parser."""
import threading

import numpy as np
import pytest

# the streams of the reference's 16 Mpixel fixture the container's flag marks as run-length packed (the reference's size rule
# replayed on its streams): all three step-0 coefficient streams (1, 65, 129) among them
MN_PACKED = {0, 1, 2, 3, 31, 33, 35, 39, 41, 43, 59, 64, 65, 67, 128, 129, 131}


def _expand(ia, coded):
    """run lengths and DC differences undone in Python: what read_compressed must give"""
    K = coded["K"]
    out = []
    for i, s in enumerate(coded["codes"]):
        if coded["packed"][i]:
            s = ia.run_length_decode(s)
        if i in (1, 2 * K + 1, 4 * K + 1):
            z = s.astype(np.int64)
            s = (np.cumsum((z >> 1) ^ -(z & 1)) & 0xFFFF).astype(np.uint16)       # zigzagDecode, running sum, low 16 bits
        out.append(s)
    return out


def _same(ia, blob):
    coded, whole = ia.read_compressed(blob, coded=True), ia.read_compressed(blob)
    for key in ("W", "H", "K", "bs"):
        assert coded[key] == whole[key]
    assert (coded["quant"] == whole["quant"]).all()
    assert np.array_equal(coded["lengths"], whole["lengths"])
    expanded = _expand(ia, coded)
    for i in range(6 * coded["K"]):
        assert np.array_equal(expanded[i], whole["codes"][i]), i
        assert coded["expect"][i] == len(whole["codes"][i]), i
    return coded


@pytest.fixture(scope="module")
def oracle_blobs(oracle):
    """every size x K x quality: 27 oracle-encoded containers"""
    blobs = []
    for K in (1, 8, 32):
        for quality in (2.0, 3.5, "max"):
            octx = oracle.OracleContext(K, 8, 0.0 if quality == "max" else quality)
            for W, H in ((8, 8), (64, 48), (1003, 517)):
                blobs.append(octx.encode_image(oracle.synth_frame(W, H, 7 + K), quant=np.ones((3, K)) if quality == "max" else None))
    return blobs


def test_container_info(mn_bytes):
    import imageexperiments_amd as ia
    assert ia.container_info(mn_bytes) == (4928, 3264, 32, 8)
    head = bytearray(mn_bytes[:14])
    assert ia.container_info(bytes(head)) == (4928, 3264, 32, 8)
    bad_magic = b"\x00" + mn_bytes[1:64]
    k0, bs9 = bytearray(head), bytearray(head)
    k0[12] = 0
    bs9[13] = 9
    for bad in (mn_bytes[:9], bad_magic, bytes(k0), bytes(bs9)):
        with pytest.raises(ia.MpcError) as e:
            ia.container_info(bad)
        assert e.value.status == ia.api.MPC_ERR_BITSTREAM


def test_coded_streams_expand_to_read_compressed(mn_bytes, oracle_blobs):
    import imageexperiments_amd as ia
    coded = _same(ia, mn_bytes)
    assert {i for i, p in enumerate(coded["packed"]) if p} == MN_PACKED
    for blob in oracle_blobs:
        _same(ia, blob)
    # a handle of the whole parser reports no packed stream
    L, C = ia.load_library(), __import__("ctypes")
    buf = np.frombuffer(mn_bytes, np.uint8)
    h = C.c_void_p()
    assert L.mpc_read_compressed(buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(h)) == 0
    assert not any(L.mpc_streams_packed(h, i) for i in range(192))
    L.mpc_streams_free(h)


def test_coded_parse_refuses_what_the_parser_refuses(mn_bytes):
    import imageexperiments_amd as ia
    for bad in (mn_bytes[:len(mn_bytes) // 2], b"\x00" + mn_bytes[1:], mn_bytes[:20]):
        for coded in (False, True):
            with pytest.raises(ia.MpcError) as e:
                ia.read_compressed(bad, coded=coded)
            assert e.value.status == ia.api.MPC_ERR_BITSTREAM


def test_coded_parse_on_eight_threads(mn_bytes, oracle_blobs):
    """ctypes releases the GIL: eight parses side by side, same results -- the function takes no process-wide lock and shares
    no state"""
    import imageexperiments_amd as ia
    blobs = [mn_bytes] + oracle_blobs
    want = [ia.read_compressed(b, coded=True) for b in blobs]
    got, errors = [None] * 8, []

    def work(k):
        try:
            got[k] = [ia.read_compressed(b, coded=True) for b in blobs]
        except Exception as e:                                        # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for mine in got:
        for a, b in zip(mine, want):
            assert a["packed"] == b["packed"] and a["expect"] == b["expect"]
            assert np.array_equal(a["lengths"], b["lengths"])
            assert all(np.array_equal(x, y) for x, y in zip(a["codes"], b["codes"]))


def test_sequence_decode_needs_a_device(mn_bytes):
    import imageexperiments_amd as ia
    ctx = ia.create_compression_context(8, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        ctx.decode_images([mn_bytes, mn_bytes])
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    with pytest.raises(ia.MpcError) as e:
        ctx.unpack_symbol_streams_device([np.zeros(0, np.uint16)] * 48, [0] * 48, [0] * 48)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    with pytest.raises(ia.MpcError) as e:
        ctx.decode_images([])
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    ctx.close()
