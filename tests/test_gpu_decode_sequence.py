"""The container decoder on the GPU (run with -m gpu): the unpack kernels (run-length expansion, DC sums) against the host's
streams, mpc_decode_image / mpc_decode_images / _device (one implementation, entered with one frame or many) against the oracle,
refusals that leave the context usable and that are exactly the host parser's and the record rule's.  Every equality is exact."""
import hashlib

import numpy as np
import pytest

import stream_cases
from container_cases import FRAMES, corpus as _corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def ctx(ia):
    return ia.create_compression_context(8, 8, 3.5, device=0)


@pytest.fixture(scope="module")
def blobs(oracle, mn_bytes):
    out = []
    for n, (W, H, K, quality) in enumerate(FRAMES):
        octx = oracle.OracleContext(K, 8, 0.0 if quality == "max" else quality)
        out.append(octx.encode_image(oracle.synth_frame(W, H, 100 + n), quant=np.ones((3, K)) if quality == "max" else None))
    out.append(mn_bytes)
    order = np.random.default_rng(20241101).permutation(len(out))
    return [out[i] for i in order]


@pytest.fixture(scope="module")
def small_blobs(blobs):
    return [b for b in blobs if len(b) < 100000]


# ---- the unpack kernels against the host ----
def _coded_form(ia, as_coded, force):
    """(coded, packed): each stream run-length coded where the encoder's size rule says so (CompressedImage.cpp:450), or -- legal
    for a decoder: the flag decides, not the rule -- wherever it is not empty"""
    coded, packed = [], []
    for s in as_coded:
        r = ia.run_length_encode(s)
        use = len(s) > 0 if force else len(r) + 4 < len(s)
        coded.append(r if use else s)
        packed.append(use)
    return coded, packed


def _host_streams(case):
    """What the host parser makes of `as_coded`: the three step-0 coefficient streams summed up the reference's way (zigzagDecode,
    running sum, low 16 bits: CompressedImage.cpp:690-705).  That is `as_held` wherever the format's 16-bit difference coding
    round-trips; a difference beyond +-32767 loses its top bit in the container (:428-446), for the reference as for everybody,
    and such a stream comes back as the wrapped sums, not as what the encoder held.  Returns (streams, DC streams that differ)."""
    K = len(case["as_coded"]) // 6
    out, lossy = list(case["as_held"]), 0
    for i in (1, 2 * K + 1, 4 * K + 1):
        z = case["as_coded"][i].astype(np.int64)
        out[i] = (np.cumsum((z >> 1) ^ -(z & 1)) & 0xFFFF).astype(np.uint16)
        lossy += not np.array_equal(out[i], case["as_held"][i])
    return out, lossy


def _unpack_equals_held(ia, ctx, case, force, lossy_dc=0):
    coded, packed = _coded_form(ia, case["as_coded"], force)
    got = ctx.unpack_symbol_streams_device(coded, packed, [len(s) for s in case["as_held"]])
    host, lossy = _host_streams(case)
    assert lossy == lossy_dc                        # everywhere else the host's streams ARE as_held
    want = np.concatenate(host) if sum(len(s) for s in host) else np.zeros(0, np.uint16)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        off = np.cumsum([0] + [len(s) for s in case["as_held"]])
        stream = int(np.searchsorted(off, at, side="right")) - 1
        raise AssertionError(f"first difference at symbol {at}: stream {stream} (packed {packed[stream]}) position {at - off[stream]}: "
                             f"{got[at]} != {want[at]}")
    return sum(packed)


@pytest.mark.parametrize("force", [False, True])
def test_unpack_stream_cases(ia, ctx, force):
    case = stream_cases.make()
    n_packed = _unpack_equals_held(ia, ctx, case, force)
    assert n_packed == (23 if force else 12)            # one of the 24 is empty; the size rule packs 12


@pytest.mark.parametrize("force", [False, True])
def test_unpack_fuzzed_streams(ia, ctx, force):
    n_packed = n_streams = 0
    # three of the 36 fuzzed step-0 coefficient streams (cases 4, 10, 11) hold jumps beyond +-32767
    for n, case in enumerate(stream_cases.fuzz_streams(777, 12)):
        n_packed += _unpack_equals_held(ia, ctx, case, force, lossy_dc=1 if n in (4, 10, 11) else 0)
        n_streams += len(case["as_held"])
    assert n_streams == 318
    if not force:
        assert n_packed == 97


def test_unpack_refusals(ia, ctx):
    """refusals the kernels reach by comparing a stream's expanded size with what the lengths stream allows, before anything is
    written; each is followed by a correct call on the same context"""
    u16 = lambda a: np.asarray(a, np.uint16)                                          # noqa: E731
    empty = [u16([])] * 5
    run = ia.run_length_encode(u16([5] * 100))

    def call(stream, expect, packed=True):
        return ctx.unpack_symbol_streams_device([u16(stream)] + empty, [packed] + [False] * 5, [expect] + [0] * 5)

    def good():
        assert np.array_equal(call(run, 100), u16([5] * 100))
    good()
    for stream, expect, packed in ((run, 101, True), (run, 99, True),                 # one more, one less than the true expansion
                                   ([7, 7], 5, True),                                 # a dangling pair: the run it announces is not there
                                   ([3, 3, 65535], 10, True),                         # a count far beyond what is allowed
                                   ([1, 2, 3], 4, False), ([1, 2, 3], 2, False)):     # not packed: the size itself
        with pytest.raises(ia.MpcError) as e:
            call(stream, expect, packed)
        assert e.value.status == ia.api.MPC_ERR_BITSTREAM, (stream, expect)
        good()
    # the positive twin of the dangling pair: what run_length_decode gives
    assert np.array_equal(ia.run_length_decode(u16([7, 7])), u16([7, 7]))
    assert np.array_equal(call([7, 7], 2), u16([7, 7]))
    assert np.array_equal(call([4, 4, 0, 4, 4, 3], 7), ia.run_length_decode(u16([4, 4, 0, 4, 4, 3])))   # a count of zero


# ---- sequences against single frames and the oracle ----
def _equal_frames(got, want):
    assert len(got) == len(want)
    for n, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, n
        assert np.array_equal(np.asarray(a), b), n


def test_sequence_equals_single_frames_and_oracle(ia, ctx, oracle, blobs):
    want = [oracle.decode_image(b) for b in blobs]
    _equal_frames([ia.decode_image(b, ctx) for b in blobs], want)
    _equal_frames(ctx.decode_images(blobs), want)
    _equal_frames([t.cpu().numpy() for t in ctx.decode_images_device(blobs)], want)
    _equal_frames(ctx.decode_images(blobs[:1]), want[:1])
    assert np.array_equal(ctx.decode_image_device(blobs[3]).cpu().numpy(), want[3])


def test_device_output_leaves_the_tail_alone(ia, ctx, oracle, blobs):
    import torch
    want = [oracle.decode_image(b) for b in blobs]
    extra = 1000
    out = [torch.full((w.size + extra,), 0xA5, dtype=torch.uint8, device="cuda:0") for w in want]
    got = ctx.decode_images_device(blobs, out=out)
    _equal_frames([t.cpu().numpy() for t in got], want)
    for t, w in zip(out, want):
        assert (t[w.size:] == 0xA5).all()
    small = [torch.empty(w.size, dtype=torch.uint8, device="cuda:0") for w in want]
    small[5] = torch.empty(want[5].size - 1, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(ia.MpcError) as e:
        ctx.decode_images_device(blobs, out=small)
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    _equal_frames(ctx.decode_images(blobs[:3]), want[:3])


def test_float_flavour(ia, oracle, blobs):
    fast = ia.create_compression_context(8, 8, 3.5, device=0).set_fast(True)
    want = [oracle.decode_image_fast(b) for b in blobs]
    _equal_frames(fast.decode_images(blobs), want)
    _equal_frames([t.cpu().numpy() for t in fast.decode_images_device(blobs)], want)
    fast.close()


def test_three_full_size_frames(ia, oracle):
    import bench
    W, H, K, q = bench.WORKLOADS["raise"]
    assert (W, H, K) == (4928, 3264, 32)
    ctx32 = ia.create_compression_context(K, 8, q, device=0)
    containers = ctx32.encode_images([bench.synth_frame(W, H, 12345 + f) for f in range(3)])
    single = [hashlib.sha256(oracle.decode_image(b).tobytes()).hexdigest() for b in containers]     # the independent answer
    assert len(set(single)) == 3
    assert [hashlib.sha256(ia.decode_image(b, ctx32).tobytes()).hexdigest() for b in containers] == single
    got = ctx32.decode_images(containers)
    assert [g.shape for g in got] == [(H, W, 3)] * 3
    assert [hashlib.sha256(g.tobytes()).hexdigest() for g in got] == single
    on_device = ctx32.decode_images_device(containers)
    assert [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in on_device] == single
    ctx32.close()


# ---- a bad frame in a sequence ----
def _bad_containers(ia, ctx, small_blobs):
    K = 8
    counts = np.zeros((2, 3), np.uint16)
    choices = np.zeros((2, 3, K), np.uint32)
    counts[0, 0] = 1
    choices[0, 0, 0] = 600 | (2 << 16)            # step 0 picks index 600 although only 510 base atoms exist
    out_of_range = ia.assemble_streams(16, 8, K, 8, ctx.quant, counts, choices)
    donor = max(small_blobs, key=len)
    return [out_of_range, donor[:len(donor) // 2], b"\x00" + donor[1:]]


def test_bad_frame_in_a_sequence(ia, ctx, oracle, small_blobs):
    good = (small_blobs * 3)[:9]
    assert len(good) == 9
    want = [oracle.decode_image(b) for b in good]
    # by the rule mpc_decode_image followed while it was a decoder of its own (read from that code: the host parser's refusal,
    # then the record check; all three MPC_ERR_BITSTREAM)
    expected = [ia.api.MPC_ERR_BITSTREAM] * 3
    for bad, status in zip(_bad_containers(ia, ctx, small_blobs), expected):
        with pytest.raises(ia.MpcError) as alone:
            ia.decode_image(bad, ctx)
        assert alone.value.status == status
        assert "frame " not in str(alone.value), str(alone.value)
        for at in (0, 4, 9):
            seq = good[:at] + [bad] + good[at:]
            for call in (ctx.decode_images, ctx.decode_images_device):
                with pytest.raises(ia.MpcError) as e:
                    call(seq)
                assert e.value.status == alone.value.status
                assert f"frame {at}:" in str(e.value), str(e.value)
                _equal_frames([np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in call(good)], want)


# ---- the decoder refuses exactly what the host parser and the record rule refuse ----
HOST_REFUSES, BLOCK_SIZE, LENGTH_ABOVE_K, RECORD_OUTSIDE, ACCEPT = range(5)


def _verdict(ia, det_rows, x):
    """What the decoder must do with container x, computed on the host from ia.read_compressed's streams (the host's own
    expansion, no part of the decoder) and the oracle's block-row table; the first rule that matches decides."""
    try:
        s = ia.read_compressed(x)
    except ia.MpcError as e:
        assert e.status == ia.api.MPC_ERR_BITSTREAM
        return HOST_REFUSES
    if s["bs"] != 8:
        return BLOCK_SIZE
    K, nb = s["K"], len(det_rows)
    lengths = s["lengths"].reshape(-1, 3).astype(np.int64)
    if (lengths > K).any():
        return LENGTH_ABOVE_K
    for ch in range(3):
        n = lengths[:, ch]
        delta = np.zeros((len(n), K), np.int64)
        for i in range(K):                      # stream i holds the tiles with more than i steps, in tile order
            live = n > i
            d = s["codes"][2 * K * ch + 2 * i].astype(np.int64)
            assert d.size == live.sum()
            delta[live, i] = d if i == 0 else (d >> 1) ^ -(d & 1)
        choice = np.cumsum(delta, axis=1)
        steps = np.arange(K)[None, :] < n[:, None]
        in_base = steps & (choice >= 0) & (choice < nb)
        # reconstruct_tile_pixel's rule (mp_kernels.hip): the dynamic dictionary is the base rows and the detail rows of every
        # base row the tile-channel chose
        size = nb + np.where(in_base, det_rows[np.clip(choice, 0, nb - 1)], 0).sum(axis=1)
        if (steps & ((choice < 0) | (choice >= size[:, None]))).any():
            return RECORD_OUTSIDE
    return ACCEPT


def test_decoder_refuses_what_the_host_refuses(ia, ctx, oracle):
    """768 damaged containers, each with exactly one expected outcome computed on the host (_verdict).  While mpc_decode_image
    was mpc::read_compressed plus three checks this held by construction; the device now does the expansion, and this test is
    what holds the decoder to the host parser.  Verdicts per container (index: host refuses, length above K, record outside, accepted): 0: 65, 3, 0, 28; 1: 49, 0, 3,
    44; 2: 28, 0, 14, 54; 5: 34, 0, 0, 62; 6: 59, 1, 0, 36; 7: 36, 0, 15, 45; 8: 67, 0, 0, 29; 10: 62, 0, 0, 34."""
    api = ia.api
    det_rows = oracle.OracleContext(1, 8, 3.5).det_rows.astype(np.int64)
    status_of = {HOST_REFUSES: api.MPC_ERR_BITSTREAM, BLOCK_SIZE: api.MPC_ERR_ARGUMENT, LENGTH_ABOVE_K: api.MPC_ERR_BITSTREAM,
                 RECORD_OUTSIDE: api.MPC_ERR_BITSTREAM}
    totals = [0] * 5
    refused = accepted = compared = 0

    def still_usable(blob):
        assert np.array_equal(ia.decode_image(blob, ctx), oracle.decode_image(blob))

    def check(x, verdict, sequences_too=False):
        nonlocal refused, accepted, compared
        totals[verdict] += 1
        if verdict == ACCEPT:
            w, h, _, _ = ia.container_info(x)
            got = ia.decode_image(x, ctx)
            assert got.shape == (h, w, 3)
            if accepted % 8 == 0:
                assert np.array_equal(got, oracle.decode_image(x))
                compared += 1
            assert ctx.decode_images([x])[0].shape == (h, w, 3)
            assert tuple(ctx.decode_images_device([x])[0].shape) == (h, w, 3)
            accepted += 1
            return
        with pytest.raises(ia.MpcError) as e:
            ia.decode_image(x, ctx)
        assert e.value.status == status_of[verdict], (verdict, str(e.value))
        assert "frame " not in str(e.value), str(e.value)
        if refused % 16 == 0 or sequences_too:
            for call in (ctx.decode_images, ctx.decode_images_device):
                with pytest.raises(ia.MpcError) as e:
                    call([x])
                assert e.value.status == status_of[verdict], (verdict, str(e.value))
                assert "frame 0:" in str(e.value), str(e.value)
        refused += 1

    for n, blob, xs in _corpus(oracle):
        assert _verdict(ia, det_rows, blob) == ACCEPT
        for x in xs:
            check(x, _verdict(ia, det_rows, x))
        if n == 5:
            still_usable(blob)                  # in the middle of the refusals
    still_usable(blob)
    assert totals == [400, 0, 4, 32, 332]
    assert (refused, accepted, compared) == (436, 332, 42)
    # The corpus leaves the block-size class empty: every flip of the header's block size also changes the tile count, and the
    # host parser refuses first.  One hand-made input to fill it: byte 13 (the block size) of a valid container set to 4.
    # The host parser refuses that too -- the lengths stream then describes a quarter of the tiles it must --, so it is
    # verdict 1 like the flips and the class stays empty.
    x = bytearray(blob)
    x[13] = 4
    x = bytes(x)
    assert _verdict(ia, det_rows, x) == HOST_REFUSES
    check(x, HOST_REFUSES, sequences_too=True)
    # A frame of one tile at either block size keeps its lengths stream whole: the host parser accepts it and the block size is
    # all that is wrong with it.
    x = bytearray(oracle.OracleContext(8, 8, 3.5).encode_image(oracle.synth_frame(4, 3, 7)))
    x[13] = 4
    x = bytes(x)
    assert _verdict(ia, det_rows, x) == BLOCK_SIZE
    check(x, BLOCK_SIZE, sequences_too=True)
    still_usable(blob)


def test_container_job_survives_a_sequence_decode(ia, oracle, small_blobs):
    import torch
    K, W, H = 16, 136, 104
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    octx = oracle.OracleContext(K, 8, 3.5)
    rgb = oracle.synth_frame(W, H, 77)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    d_rgb = torch.from_numpy(rgb).cuda()
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, (H + 7) // 8, d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    want = bytes(octx.encode_image(rgb))
    decoded = [oracle.decode_image(b) for b in small_blobs]
    ctx.container_job_begin(0, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    _equal_frames(ctx.decode_images(small_blobs), decoded)                  # between begin and tables
    ctx.container_job_tables(0)
    _equal_frames([t.cpu().numpy() for t in ctx.decode_images_device(small_blobs)], decoded)   # between tables and collect
    assert bytes(ctx.container_job_collect(0)) == want
    ctx.close()
