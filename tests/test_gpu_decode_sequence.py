"""The sequence decoder on the GPU (run with -m gpu): the unpack kernels (run-length expansion, DC sums) against the host's
streams, mpc_decode_images / _device against single-frame decodes and the oracle, refusals that leave the context usable.
Every equality is exact."""
import hashlib

import numpy as np
import pytest

import stream_cases

pytestmark = pytest.mark.gpu

# (width, height, K, quality) of the oracle-encoded containers: mixed geometry, K and quality, more frames than slots
FRAMES = [(8, 8, 1, 2.0), (16, 8, 8, 3.5), (200, 120, 32, "max"), (1003, 517, 32, 3.5), (1920, 1080, 8, 6.0), (8, 8, 32, 6.0),
          (16, 8, 1, "max"), (200, 120, 8, 2.0), (1003, 517, 1, 6.0), (1920, 1080, 1, 2.0), (200, 120, 1, 3.5), (1003, 517, 8, "max")]


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


def test_three_full_size_frames(ia):
    import bench
    W, H, K, q = bench.WORKLOADS["raise"]
    assert (W, H, K) == (4928, 3264, 32)
    ctx32 = ia.create_compression_context(K, 8, q, device=0)
    containers = ctx32.encode_images([bench.synth_frame(W, H, 12345 + f) for f in range(3)])
    single = [hashlib.sha256(ia.decode_image(b, ctx32).tobytes()).hexdigest() for b in containers]
    assert len(set(single)) == 3
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
    for bad in _bad_containers(ia, ctx, small_blobs):
        with pytest.raises(ia.MpcError) as alone:
            ia.decode_image(bad, ctx)
        for at in (0, 4, 9):
            seq = good[:at] + [bad] + good[at:]
            for call in (ctx.decode_images, ctx.decode_images_device):
                with pytest.raises(ia.MpcError) as e:
                    call(seq)
                assert e.value.status == alone.value.status
                assert f"frame {at}:" in str(e.value), str(e.value)
                _equal_frames([np.asarray(x.cpu()) if hasattr(x, "cpu") else x for x in call(good)], want)


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
