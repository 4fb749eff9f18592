"""The host half of the sequence decoder (no GPU): the container's header alone, and the serial half of readCompressed on its
own -- the streams as entropy-decoded, still run-length packed and difference coded -- against the whole parser."""
import hashlib
import threading

import numpy as np
import pytest

import container_cases

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


# Per damaged-container corpus (index in container_cases.FRAMES): inputs of 96 that read_compressed, read_compressed(coded=True)
# and container_info refuse, and the SHA-256 over `lengths` and all `codes` (their bytes, in that order, input after input) of
# the inputs read_compressed accepts.  Recorded from the library as it was before the host coder was split into three sources.
CORPUS_PARSE = {
    0: (65, 65, 21, "13d8ffcd4da55bba4673afb8af161419d9d0275152a253c5e3b13af134acb036"),
    1: (49, 49, 2, "8c2a3836c712ab78158aa368b6faba295ce212643b012ee0148ab7055875dbc3"),
    2: (28, 22, 1, "4b608623be3785f9f5ec512fd48e4f8dab88b64bc1f7304d488abb7f55dd8764"),
    5: (34, 34, 2, "0676e7094e072f1b3700c67015682bac886144509224deb2754c955136ac701e"),
    6: (59, 59, 17, "d3a009aa2f32158035ece947218dafc2f76f6b2d244dc1cf478181dc4bdce3a7"),
    7: (36, 28, 3, "1a907f268dddf2b81f070ba17bdfa63f580dea73fb81497aab9a9d08f2c818cc"),
    8: (67, 44, 5, "bb759e6f5f44dfa3e4b6554b43f6516cc142c3ce5190f68069808c7a323fc70f"),
    10: (62, 51, 5, "19af970485fc713b21021e0adfb3c9b62d78bc1d0ee8d92f3f79de9c825ce3d1"),
}


def test_parser_verdicts_and_streams_on_the_damaged_corpus(oracle):
    """The 768 damaged containers the device decoder is held to (test_gpu_decode_sequence), on the host parser alone: which of
    them each entry point refuses (always MPC_ERR_BITSTREAM), and what read_compressed makes of the rest, pinned to the bytes."""
    import imageexperiments_amd as ia

    def refuses(call, x):
        try:
            return False, call(x)
        except ia.MpcError as e:
            assert e.status == ia.api.MPC_ERR_BITSTREAM
            return True, None

    seen = {}
    for n, blob, xs in container_cases.corpus(oracle):
        assert len(xs) == 96
        digest = hashlib.sha256()
        whole = coded = info = 0
        for x in xs:
            refused, s = refuses(ia.read_compressed, x)
            whole += refused
            if not refused:
                digest.update(s["lengths"].tobytes())
                for c in s["codes"]:
                    digest.update(c.tobytes())
            coded += refuses(lambda b: ia.read_compressed(b, coded=True), x)[0]
            info += refuses(ia.container_info, x)[0]
        seen[n] = (whole, coded, info, digest.hexdigest())
        print(n, seen[n])
    assert seen == CORPUS_PARSE
    assert sum(v[0] for v in seen.values()) == 400


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
