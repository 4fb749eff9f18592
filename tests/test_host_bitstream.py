"""Host entropy stage of the PRODUCT (libmpcodec.so, C++) against the golden container and the oracle.
The property tests mirror the reference's Testing/HuffmanTest.cpp and BitBufferTests.cpp (round trips, code
length consistency); the golden test is stronger than anything the reference holds: byte identity."""
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd
    return imageexperiments_amd


def test_mn_reencode_is_byte_exact(ia, mn_bytes):
    """readCompressed -> writeCompressed of Data/r0c1de5e1t_3_5.mn through the C ABI reproduces the file."""
    st = ia.read_compressed(mn_bytes)
    assert (st["W"], st["H"], st["K"], st["bs"]) == (4928, 3264, 32, 8)
    assert len(st["lengths"]) == 753984
    out = ia.write_compressed(st["W"], st["H"], st["K"], st["bs"], st["quant"].astype(np.float64), st["lengths"], st["codes"])
    assert out == mn_bytes


def test_mn_streams_equal_oracle_parse(ia, oracle, mn_bytes):
    a = ia.read_compressed(mn_bytes)
    b = oracle.read_compressed(mn_bytes)
    assert (a["quant"] == b["quant"]).all()
    assert (a["lengths"] == b["lengths"]).all()
    for x, y in zip(a["codes"], b["codes"]):
        assert (x == y).all()


def test_decode_without_a_device_fails_loudly(ia, mn_bytes):
    """Tile reconstruction exists on the device only: a host-only context gets MPC_ERR_NO_DEVICE, never a CPU decode."""
    ctx = ia.create_compression_context(32, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        ia.decode_image(mn_bytes, ctx)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    ctx.close()


def _oracle_huffman(oracle, data):
    import ctypes as C
    L = oracle.lib()
    b = oracle.Bits()
    L.mpo_bits_init(C.byref(b))
    a = np.ascontiguousarray(data, np.uint16)
    L.mpo_huffman_encode(oracle._u16p(a), a.size, C.byref(b))
    n = C.c_size_t(0)
    p = L.mpo_bits_save(C.byref(b), C.byref(n))
    out = bytes(C.string_at(p, n.value))
    oracle._libc_free(p)
    L.mpo_bits_free(C.byref(b))
    return out


def _partitions(n, maxpart=None):
    maxpart = maxpart or n
    if n == 0:
        yield []
        return
    for first in range(min(n, maxpart), 0, -1):
        for rest in _partitions(n - first, first):
            yield [first] + rest


def test_huffman_empty(ia, oracle):
    """HuffmanTest.cpp EmptyTest: empty input encodes to the lone pseudo-EOF and decodes to nothing."""
    blob = ia.huffman_encode([])
    assert blob == _oracle_huffman(oracle, [])
    assert ia.huffman_decode(blob).size == 0


def test_huffman_all_frequency_profiles_of_ten(ia, oracle):
    """HuffmanTest.cpp BasicTest: every integer partition of 10 as a frequency profile -> many tree shapes."""
    for part in _partitions(10):
        data = np.concatenate([np.full(f, 100 + 7 * i, np.uint16) for i, f in enumerate(part)])
        np.random.default_rng(len(part)).shuffle(data)
        blob = ia.huffman_encode(data)
        assert blob == _oracle_huffman(oracle, data), part
        assert (ia.huffman_decode(blob) == data).all(), part


def test_huffman_all_ones_symbol_vs_pseudo_eof(ia, oracle):
    """HuffmanTest.cpp BasicTest2: a real symbol equal to the all-ones mask next to the pseudo-EOF."""
    for width in (1, 3, 8, 13, 16):
        top = (1 << width) - 1
        data = np.array([top, 0, top, top, 1 % (top + 1), top], np.uint16)
        blob = ia.huffman_encode(data)
        assert blob == _oracle_huffman(oracle, data)
        assert (ia.huffman_decode(blob) == data).all()


def test_huffman_large_and_many_ties(ia, oracle):
    """HuffmanTest.cpp LargeTest (100k symbols) + wide alphabets with many equal frequencies, where the
    MSVC hash-order tie-breaking decides the code lengths."""
    rng = np.random.default_rng(2)
    cases = [rng.integers(0, 300, 100000).astype(np.uint16),
             np.arange(5000, dtype=np.uint16),                         # all frequencies equal, 5000 leaves: rehashes
             np.repeat(np.arange(700, dtype=np.uint16), 3),
             (rng.geometric(0.02, 50000) % 9000).astype(np.uint16),
             rng.integers(0, 65536, 3000).astype(np.uint16)]
    for data in cases:
        blob = ia.huffman_encode(data)
        assert blob == _oracle_huffman(oracle, data)
        assert (ia.huffman_decode(blob) == data).all()


def test_huffman_heap_order_on_many_small_tie_heavy_alphabets(ia, oracle):
    """The reference's priority_queue orders by frequency alone: among equal frequencies the heap algorithm itself decides, and the
    product restates libstdc++'s push_heap / pop_heap step for step on packed words (host_bitstream.cpp: FrequencyHeap).  Every heap
    size from 1 to 130 leaves (both parities of every level) and a few hundred random larger ones, frequencies from a handful of
    values so that almost everything ties, against the oracle's own heap."""
    rng = np.random.default_rng(77)
    sizes = list(range(1, 131)) + [int(x) for x in rng.integers(131, 2500, 120)]
    for n in sizes:
        symbols = rng.choice(65536, size=n, replace=False).astype(np.uint16)
        counts = rng.choice([1, 1, 1, 2, 2, 3, 5, 8], size=n)
        data = np.repeat(symbols, counts)
        rng.shuffle(data)
        blob = ia.huffman_encode(data)
        assert blob == _oracle_huffman(oracle, data), n
    data = np.repeat(rng.choice(65536, size=40000, replace=False).astype(np.uint16), 1)      # 40 000 leaves, all ties
    assert ia.huffman_encode(data) == _oracle_huffman(oracle, data)


def test_huffman_decode_fast_paths(ia, oracle):
    """The decoder's fast loop (bit buffer, one- or two-symbol table, second-level tables for codes longer than the window) and
    its fall-backs: geometric frequencies (code lengths up to the twenties: sub-tables), Fibonacci frequencies (lengths beyond 26:
    the length-by-length route), large flat alphabets (every code longer than the window), long runs of one symbol (two symbols
    per look-up), and streams shorter than the fast loop's 16 bytes.  Encoded bytes equal the oracle's, decoding returns the data,
    and a few flipped bits never crash (an error or other symbols, like the reference)."""
    rng = np.random.default_rng(5)
    cases = []
    for ratio in (0.5, 0.62, 0.7, 0.8):                                   # geometric: P(symbol k) ~ ratio^k
        p = ratio ** np.arange(40)
        cases.append(rng.choice(40, size=60000, p=p / p.sum()).astype(np.uint16) * 37)
    fib = [1, 1]
    while len(fib) < 32:
        fib.append(fib[-1] + fib[-2])
    cases.append(np.repeat(np.arange(32, dtype=np.uint16), np.minimum(fib, 200000)).astype(np.uint16))   # very long codes
    rng.shuffle(cases[-1])
    cases.append(rng.integers(0, 5000, 200000).astype(np.uint16))           # flat: 12-13 bit codes only
    cases.append(rng.integers(0, 60000, 30000).astype(np.uint16))           # nearly all symbols distinct
    cases.append(np.where(rng.random(300000) < 0.97, 7, rng.integers(0, 300, 300000)).astype(np.uint16))
    cases.append(np.array([3, 3, 1], np.uint16))
    cases.append(np.arange(9, dtype=np.uint16))
    for data in cases:
        blob = ia.huffman_encode(data)
        assert blob == _oracle_huffman(oracle, data)
        assert (ia.huffman_decode(blob) == data).all()
        raw = bytearray(blob)
        for _ in range(8):                                                   # corrupt: an error or different symbols, never a crash
            bad = bytearray(raw)
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
            try:
                ia.huffman_decode(bytes(bad))
            except ia.MpcError:
                pass


def test_huffman_corrupt_stream_is_an_error(ia):
    """HuffmanTest.cpp CorruptStreamTest: truncated data -> 'Invalid bitstream' (status, not an exception pointer)."""
    data = np.random.default_rng(3).integers(0, 50, 2000).astype(np.uint16)
    blob = ia.huffman_encode(data)
    with pytest.raises(ia.MpcError) as e:
        ia.huffman_decode(blob[:len(blob) // 2])
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM


@pytest.mark.parametrize("case", range(25))
def test_rle_round_trip(ia, case):
    """HuffmanTest.cpp RLETest x25: random run structures round-trip."""
    rng = np.random.default_rng(case)
    runs = rng.integers(1, 1 + [1, 2, 5, 40, 400][case % 5], 200)
    vals = rng.integers(0, [2, 3, 10, 1000, 65536][(case // 5) % 5], 200)
    data = np.repeat(vals, runs).astype(np.uint16)
    enc = ia.run_length_encode(data)
    assert (ia.run_length_decode(enc) == data).all()


def test_rle_long_sequences(ia, oracle):
    """HuffmanTest.cpp LongSequences: runs >= 0x8000 are split."""
    import ctypes as C
    for n in (0x7FFF, 0x8000, 0x8001, 0x10000, 0x18005):
        data = np.concatenate([np.full(n, 7, np.uint16), np.array([7, 9, 9], np.uint16)])
        enc = ia.run_length_encode(data)
        assert (ia.run_length_decode(enc) == data).all()
        v = oracle.U16V()
        oracle.lib().mpo_rle_encode(oracle._u16p(data), data.size, C.byref(v))
        ref = np.ctypeslib.as_array(v.d, shape=(v.n,)).copy()
        oracle.lib().mpo_u16v_free(C.byref(v))
        assert (enc == ref).all()


def test_write_compressed_equals_oracle_on_random_streams(ia, oracle):
    """whole containers (RLE decision, DC differencing, Huffman-or-Golomb incl. the Golomb branch)."""
    rng = np.random.default_rng(11)
    for K, tiles_x, tiles_y in ((4, 5, 3), (8, 9, 7), (32, 6, 6)):
        W, H = tiles_x * 8 - 3, tiles_y * 8
        T = tiles_x * tiles_y
        counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
        choices = np.zeros((T, 3, K), np.uint32)
        delta = rng.integers(0, 3000, (T, 3, K))
        coef = (rng.geometric(0.05, (T, 3, K)) - 1) % 4000        # geometric: Golomb wins on some streams
        choices[:] = delta | (coef << 16)
        quant = rng.integers(1, 500, (3, K)).astype(np.float64)
        blob = ia.assemble_streams(W, H, K, 8, quant, counts, choices)
        lengths = counts.reshape(-1)
        codes = [[] for _ in range(6 * K)]
        for t in range(T):
            for ch in range(3):
                for i in range(counts[t, ch]):
                    codes[2 * K * ch + 2 * i].append(int(delta[t, ch, i]))
                    codes[2 * K * ch + 2 * i + 1].append(int(coef[t, ch, i]))
        st = dict(W=W, H=H, K=K, bs=8, quant=quant.astype(np.uint16), lengths=lengths,
                  codes=[np.array(c, np.uint16) for c in codes])
        assert blob == oracle.write_compressed(st)
        back = ia.read_compressed(blob)
        assert (back["lengths"] == lengths).all()
        for x, y in zip(back["codes"], st["codes"]):
            assert (x == y).all()


def test_invalid_container_is_an_error(ia, mn_bytes):
    with pytest.raises(ia.MpcError) as e:
        ia.read_compressed(b"\x00" * 64)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM
    with pytest.raises(ia.MpcError):
        ia.read_compressed(mn_bytes[:1000])


@pytest.mark.parametrize("size,K,bpp,threads", [((96, 64), 8, 3.5, "1"), ((72, 40), 32, 3.5, "3"), ((130, 50), 16, 2.0, "16"),
                                                ((8, 8), 4, 6.0, "2")])
def test_records_to_container_equals_oracle(ia, oracle, monkeypatch, size, K, bpp, threads):
    """mpc_assemble_streams (records -> container in one pass per (channel, step), worker pool): bytes equal the oracle's
    encodeImage on the same records, whatever the number of host threads"""
    monkeypatch.setenv("MPC_HOST_THREADS", threads)
    w, h = size
    rgb = oracle.synth_frame(w, h, 7 + K)
    octx = oracle.OracleContext(K, 8, bpp)
    counts, delta, coef, _, _ = octx.encode_tiles(rgb)
    choices = delta.astype(np.uint32) | (coef.astype(np.uint32) << 16)
    blob = ia.assemble_streams(w, h, K, 8, octx.quant, counts, choices)
    assert bytes(blob) == bytes(octx.encode_image(rgb))
    # records in planar order ([3][K][tiles], mpc_assemble_planar_streams) give the same container
    planar = np.ascontiguousarray(choices.reshape(-1, 3, K).transpose(1, 2, 0))
    assert bytes(ia.api.assemble_planar_streams(w, h, K, 8, octx.quant, counts, planar)) == bytes(blob)


def _small_container(oracle, W=40, H=24, K=4):
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return oracle.OracleContext(K, 8, 3.5).encode_image(rgb)


def test_truncated_and_corrupted_containers_are_errors_not_crashes(ia, oracle, mn_bytes):
    """the parser must not trust the header.  Every prefix / bit flip either parses to streams that are
    consistent with the header (lengths == 3 * tiles, every stream its expected length) or returns
    MPC_ERR_BITSTREAM / MPC_ERR_ALLOC -- no exception may cross the C ABI and nothing may be sized from a lying field."""
    blob = _small_container(oracle)
    st = ia.read_compressed(blob)
    tiles = ((st["W"] + 7) // 8) * ((st["H"] + 7) // 8)
    assert len(st["lengths"]) == 3 * tiles
    bad = 0
    for cut in list(range(0, 64)) + list(range(64, len(blob), 7)):
        try:
            s = ia.read_compressed(blob[:cut])
        except ia.MpcError as e:
            assert e.status in (ia.api.MPC_ERR_BITSTREAM, ia.api.MPC_ERR_ALLOC)
            bad += 1
            continue
        t = ((s["W"] + 7) // 8) * ((s["H"] + 7) // 8)
        assert len(s["lengths"]) == 3 * t
    assert bad > 0
    rng = np.random.default_rng(3)
    for _ in range(400):
        b = bytearray(blob)
        for _k in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        try:
            s = ia.read_compressed(bytes(b))
        except ia.MpcError as e:
            assert e.status in (ia.api.MPC_ERR_BITSTREAM, ia.api.MPC_ERR_ALLOC)
            continue
        t = ((s["W"] + 7) // 8) * ((s["H"] + 7) // 8)
        assert len(s["lengths"]) == 3 * t
    # a header that claims a gigantic frame over a few bytes of data
    huge = bytearray(mn_bytes[:4096])
    huge[4:8] = (0x7FFFFFF0).to_bytes(4, "big")
    huge[8:12] = (0x7FFFFFF0).to_bytes(4, "big")
    with pytest.raises(ia.MpcError):
        ia.read_compressed(bytes(huge))
    with pytest.raises(ia.MpcError):
        ia.read_compressed(mn_bytes[: len(mn_bytes) // 2])


def test_symbol_streams_direct_and_planned_routes_equal_the_oracle(ia, oracle):
    """The container from assembled streams, on adversarial streams (tests/stream_cases.py): the host's direct route, and the
    route the device-side entropy stage takes (statistics -> plan_stream -> codes at planned offsets -> or_bits) with the
    device's share done on the host, both against the oracle's writeCompressed."""
    import stream_cases
    c = stream_cases.make()
    q = stream_cases.quant(c["K"])
    want = oracle.write_compressed(dict(W=c["W"], H=c["H"], K=c["K"], bs=c["bs"], quant=q, lengths=c["counts"], codes=c["as_held"]))
    direct = ia.assemble_symbol_streams(c["W"], c["H"], c["K"], c["bs"], q, c["counts"], c["as_coded"])
    assert direct == want
    planned = ia.assemble_symbol_streams(c["W"], c["H"], c["K"], c["bs"], q, c["counts"], c["as_coded"], by_plan=True)
    assert planned == want


def test_planned_route_with_symbols_that_first_appear_millions_of_positions_in(ia, oracle):
    """plan_stream orders a stream's symbols by first appearance with a radix sort, 11 bits of the position a pass: first
    appearances beyond 2^22 take the third pass, alphabets under 128 symbols a comparison sort -- both against the oracle."""
    import stream_cases
    rng = np.random.default_rng(5)
    W = H = 8 * 900
    K, tiles = 2, 900 * 900
    late = np.concatenate([rng.integers(0, 3, 4_300_000), rng.permutation(np.arange(3, 700)), rng.integers(0, 700, 5000)]).astype(np.uint16)
    few = np.concatenate([np.zeros(4_250_000, np.uint16), rng.integers(0, 90, 20000).astype(np.uint16)])   # long runs: run-length coded
    streams = [late, rng.integers(0, 50, 1000).astype(np.uint16), few] + [np.zeros(0, np.uint16)] * (6 * K - 3)
    assert sum(len(x) for x in streams) <= 2 * 3 * tiles * K
    counts = rng.integers(0, K + 1, 3 * tiles).astype(np.uint16)
    q = stream_cases.quant(K)
    planned = ia.assemble_symbol_streams(W, H, K, 8, q, counts, streams, by_plan=True)
    direct = ia.assemble_symbol_streams(W, H, K, 8, q, counts, streams)
    assert planned == direct
    # the oracle takes the DC slot (stream 1) before differencing: an empty one needs none
    streams_o = [late, np.zeros(0, np.uint16), few] + [np.zeros(0, np.uint16)] * (6 * K - 3)
    want = oracle.write_compressed(dict(W=W, H=H, K=K, bs=8, quant=q, lengths=counts, codes=streams_o))
    assert ia.assemble_symbol_streams(W, H, K, 8, q, counts, streams_o, by_plan=True) == want


def test_container_jobs_refuse_misuse_without_touching_a_device(ia):
    """mpc_container_job_*: a host-only context has no device (begin), a slot that has not begun has no tables to build, one
    without tables nothing to collect, and slots are bounded -- status codes, no HIP call."""
    ctx = ia.create_compression_context(8, 8, 3.5, device=-1)
    with pytest.raises(ia.MpcError) as e:
        ctx.container_job_begin(0, 1, 1, 64, 64)
    assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    ctx.container_job_cancel(0)                                   # an idle slot: no-op
    ctx.container_job_cancel(5)
    with pytest.raises(ia.MpcError):
        ctx.container_job_cancel(6)
    for call in (lambda: ctx.container_job_tables(0), lambda: ctx.container_job_collect(0), lambda: ctx.container_job_tables(99),
                 lambda: ctx.container_job_collect(-1)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    ctx.close()
