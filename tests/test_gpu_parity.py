"""GPU parity (run with -m gpu): the HIP path, called through the C ABI (libmpcodec.so), against the CPU
oracle on the same inputs.  Integer fields must be bit-exact; the residual energy is compared at the
north_star's 1e-5 relative tolerance AND bit-exactly (the kernel keeps the oracle's operation order)."""
import numpy as np
import pytest

from parity_compare import REL_TOL_ENERGY, compare as _compare
from pursuit_cases import adversarial_vectors as _adversarial_vectors, degenerate_frames, nan_vectors, near_tie_vectors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    return torch


@pytest.fixture(scope="module")
def ctx32(gpu):
    import imageexperiments_amd as ia
    return ia.create_compression_context(32, 8, 3.5, device=0)


@pytest.fixture(scope="module")
def ctx8(gpu):
    import imageexperiments_amd as ia
    return ia.create_compression_context(8, 8, 3.5, device=0)


def _oracle_records(octx, rgb, quant=None):
    """oracle records re-ordered to the C ABI's order for a full-height stripe (identical: tx*tilesY + ty)."""
    return octx.encode_tiles(rgb, quant=quant)


def test_dictionary_on_host_matches_oracle(ctx32, octx32):
    base, rows, det = ctx32.dictionary()
    assert (base.view(np.uint64) == octx32.base.view(np.uint64)).all()
    assert (rows == octx32.det_rows).all()
    for ch in range(3):
        assert (det[ch].view(np.uint64) == octx32.det[ch].view(np.uint64)).all()
    assert (ctx32.quant == octx32.quant).all()


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_calc_mp_vectors_bit_exact(ctx32, octx32, channel):
    """matching::CalcMPDynamic on raw vectors: several magnitudes, all steps up to K=32."""
    rng = np.random.default_rng(100 + channel)
    vecs = []
    for scale in (0.4, 3.0, 40.0, 400.0, 2000.0):
        vecs.append(rng.standard_normal((40, 64)) * scale)
    vecs.append(np.zeros((2, 64)))                                  # all projections zero -> index -1 path (:50-54)
    vecs.append(np.full((2, 64), 255.0))                            # pure DC
    vecs.append(rng.integers(0, 256, (40, 64)).astype(np.float64))  # pixel-like
    v = np.vstack(vecs)
    counts, choices, energy, swept = ctx32.calc_mp(channel, v)
    for i in range(v.shape[0]):
        cnt, d, k, res, S = octx32.calc_mp(channel, v[i])
        assert counts[i] == cnt, i
        n = min(cnt + 1, 32)
        assert (choices["deltaId"][i, :n] == d[:n]).all(), i
        assert (choices["intCoeff"][i, :n] == k[:n]).all(), i
        assert swept[i] == S
        assert energy[i] == float((res * res).sum()) or np.isclose(energy[i], (res * res).sum(), rtol=REL_TOL_ENERGY)


def test_calc_mp_unit_quant_deep_pursuit(ctx32, octx32):
    """quant = 1 everywhere (Compression.cpp 'max' mode / -s mode): every step survives, deep block lists,
    duplicates of the DC block."""
    rng = np.random.default_rng(5)
    v = rng.integers(0, 256, (64, 64)).astype(np.float64)
    q = np.ones(32)
    counts, choices, energy, swept = ctx32.calc_mp(0, v, quant_k=q)
    for i in range(v.shape[0]):
        cnt, d, k, res, S = octx32.calc_mp(0, v[i], quant=q)
        assert counts[i] == cnt
        n = min(cnt + 1, 32)
        assert (choices["deltaId"][i, :n] == d[:n]).all()
        assert (choices["intCoeff"][i, :n] == k[:n]).all()
        assert swept[i] == S


@pytest.mark.parametrize("size", [(64, 48), (70, 50), (8, 8), (3, 5), (129, 17)])
def test_encode_tiles_small_images(ctx32, octx32, oracle, size):
    """whole small frames incl. sizes that are not multiples of 8 (zero fill, CompressedImage.cpp:548-552)."""
    W, H = size
    rgb = oracle.synth_frame(W, H, 12345)
    _compare(ctx32.encode_tiles(rgb), _oracle_records(octx32, rgb), 32)


def test_encode_tiles_k8_random_noise(ctx8, oracle):
    octx8 = oracle.OracleContext(8, 8, 3.5)
    rng = np.random.default_rng(9)
    rgb = rng.integers(0, 256, (40, 72, 3)).astype(np.uint8)
    _compare(ctx8.encode_tiles(rgb), _oracle_records(octx8, rgb), 8)


def test_encode_tiles_quality_sweep(gpu, oracle):
    """BASELINE config 3 sweeps quality 2.0 .. 6.0; small frame here, the tables differ per quality."""
    import imageexperiments_amd as ia
    rgb = oracle.synth_frame(96, 64, 777)
    for bpp in (2.0, 4.5, 6.0):
        c = ia.create_compression_context(32, 8, bpp, device=0)
        o = oracle.OracleContext(32, 8, bpp)
        _compare(c.encode_tiles(rgb), _oracle_records(o, rgb), 32)
        c.close()


def test_row_stripes_equal_full_frame(ctx32, oracle):
    """tile rows [a,b) of a frame == the same rows of the full-frame result (the multi-GPU sharding unit)."""
    rgb = oracle.synth_frame(80, 72, 4242)       # 10 x 9 tiles
    full = ctx32.encode_tiles(rgb)
    tx, ty = 10, 9
    for a, b in ((0, 4), (4, 9), (8, 9)):
        part = ctx32.encode_tiles(rgb, a, b)
        rows = b - a
        for arr_full, arr_part in zip(full, part):
            f = arr_full.reshape((tx, ty) + arr_full.shape[1:])[:, a:b]
            assert (f.reshape((tx * rows,) + arr_full.shape[1:]) == arr_part).all()


def test_histogram_matches_numpy(gpu, ctx32, oracle):
    """per-stream symbol histograms (the RCCL all-reduce operand) == numpy bincount of the records."""
    import torch
    rgb = oracle.synth_frame(160, 96, 31)
    counts, choices, energy, swept = ctx32.encode_tiles(rgb)
    T, K = counts.shape[0], 32
    d_counts = torch.from_numpy(counts.astype(np.int16)).cuda()
    d_choices = torch.from_numpy(choices.view(np.uint32).astype(np.int64).astype(np.int32).reshape(T, 3, K)).cuda()
    d_hist = torch.zeros((1 + 6 * K, 8192), dtype=torch.int32, device="cuda")
    ctx32.histogram_device(d_counts.data_ptr(), d_choices.data_ptr(), T, d_hist.data_ptr())
    torch.cuda.synchronize()
    hist = d_hist.cpu().numpy()
    ref = np.zeros_like(hist)
    ref[0] = np.bincount(counts.reshape(-1), minlength=8192)
    for ch in range(3):
        for i in range(K):
            m = counts[:, ch] > i
            ref[1 + 2 * K * ch + 2 * i] = np.bincount(choices["deltaId"][m, ch, i], minlength=8192)
            ref[2 + 2 * K * ch + 2 * i] = np.bincount(choices["intCoeff"][m, ch, i], minlength=8192)
    assert (hist == ref).all()


@pytest.mark.parametrize("size,K,bpp", [((64, 48), 32, 3.5), ((70, 50), 8, 3.5), ((129, 17), 16, 2.0), ((256, 256), 32, 3.5)])
def test_encode_image_bytes_equal_oracle(gpu, oracle, size, K, bpp):
    """BASELINE metric 'bitstream byte-diff vs CPU': compressed::encodeImage (device tiles + host entropy
    stage) emits exactly the oracle's bytes; the product's decoder inverts it like the oracle's."""
    import imageexperiments_amd as ia
    W, H = size
    rgb = oracle.synth_frame(W, H, 2024)
    ctx = ia.create_compression_context(K, 8, bpp, device=0)
    octx = oracle.OracleContext(K, 8, bpp)
    blob = ctx.encode_image(rgb)
    ref = octx.encode_image(rgb)
    assert blob == ref
    img = ia.decode_image(blob, ctx)
    assert (img == oracle.decode_image(ref)).all()
    assert img.shape == rgb.shape
    assert ia.calculate_psnr(rgb, img) > 25.0
    ctx.close()


def test_max_quality_mode_overrides_quant(gpu, oracle):
    """Compression.cpp:104-110 'max': every quant step forced to 1.0 after context creation."""
    import imageexperiments_amd as ia
    rgb = oracle.synth_frame(40, 24, 5)
    ctx = ia.create_compression_context(16, 8, 0.0, device=0)
    ones = np.ones((3, 16))
    ctx.set_quant(ones)
    octx = oracle.OracleContext(16, 8, 0.0)
    assert ctx.encode_image(rgb, quant=ones) == octx.encode_image(rgb, quant=ones)
    ctx.close()


def test_full_size_1080p_properties(gpu, oracle):
    """BASELINE configs[1] at full size (1920x1080, K=8, q=3.5): too large for the oracle in a test, so
    size-independent properties: (1) a sample of tile columns equals the oracle exactly, (2) swept rows follow
    from the records, (3) decode(encode) reproduces the frame to the PSNR the sample predicts, (4) row stripes
    compose, (5) the run is deterministic."""
    import imageexperiments_amd as ia
    W, H, K = 1920, 1080, 8
    rgb = oracle.synth_frame(W, H, 12345)
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    counts, choices, energy, swept = ctx.encode_tiles(rgb)
    tiles_x, tiles_y = 240, 135
    assert counts.shape == (tiles_x * tiles_y, 3)
    # (1) oracle on 6 tile columns spread over the frame
    octx = oracle.OracleContext(K, 8, 3.5)
    for tx in (0, 57, 119, 180, 238, 239):
        oc, od, ok, oe, os_ = octx.encode_tiles(rgb, tx_begin=tx, tx_end=tx + 1)
        sl = slice(tx * tiles_y, (tx + 1) * tiles_y)
        assert (counts[sl] == oc[sl]).all()
        valid = np.arange(K)[None, None, :] <= np.minimum(oc[sl][:, :, None], K - 1)
        assert (choices["deltaId"][sl][valid] == od[sl][valid]).all()
        assert (choices["intCoeff"][sl][valid] == ok[sl][valid]).all()
        assert (swept[sl] == os_[sl]).all()
        assert (energy[sl].view(np.uint64) == oe[sl].view(np.uint64)).all()
    # (2) swept rows recomputed from the records: sum over sweeps of 510 + rows of the unlocked blocks
    base, rows, det = ctx.dictionary()
    rng = np.random.default_rng(0)
    for t in rng.integers(0, counts.shape[0], 300):
        for ch in range(3):
            c = int(counts[t, ch])
            ids, cur, total, extra = [], 0, 0, 0
            for i in range(min(c + 1, K)):
                total += 510 + extra
                if i < c:
                    d = int(choices["deltaId"][t, ch, i])
                    cur = d if i == 0 else cur + ((d >> 1) ^ -(d & 1))
                    if cur < 510:
                        extra += int(rows[cur])
            assert total == swept[t, ch]
    # (3) container round trip
    blob = ia.assemble_streams(W, H, K, 8, ctx.quant, counts, choices.view(np.uint32))
    img = ia.decode_image(blob, ctx)
    assert img.shape == rgb.shape
    psnr = ia.calculate_psnr(rgb, img)
    assert 30.0 < psnr < 60.0
    back = ia.read_compressed(blob)
    assert (back["lengths"].reshape(-1, 3) == counts).all()
    # (4) stripes compose, (5) determinism
    a, b = 0, 67
    part = ctx.encode_tiles(rgb, a, b)
    f = counts.reshape(tiles_x, tiles_y, 3)[:, a:b].reshape(-1, 3)
    assert (part[0] == f).all()
    again = ctx.encode_tiles(rgb)
    assert (again[0] == counts).all() and (again[1] == choices).all()
    ctx.close()


def test_device_decoder_equals_oracle_on_golden_mn(gpu, oracle, ctx32, mn_bytes):
    """decodeImage with the tile reconstruction on the device reproduces the oracle's decode of the
    reference's own 16 Mpixel fixture pixel for pixel (and hence 39.07 dB vs the committed JPEG)."""
    import hashlib
    import imageexperiments_amd as ia
    img = ia.decode_image(mn_bytes, ctx32)
    ref = oracle.decode_image(mn_bytes)
    assert img.shape == (3264, 4928, 3)
    assert (img == ref).all()
    assert hashlib.sha256(img.tobytes()).hexdigest() == hashlib.sha256(ref.tobytes()).hexdigest()
    # the stream's own K and tables are used: a context of another K decodes it to the same pixels
    other = ia.create_compression_context(8, 8, 5.0, device=0)
    assert (ia.decode_image(mn_bytes, other) == ref).all()
    other.close()
    # decoding leaves the context's own tables untouched
    rgb = oracle.synth_frame(64, 48, 1)
    assert ctx32.encode_image(rgb) == oracle.OracleContext(32, 8, 3.5).encode_image(rgb)


def test_device_decoder_rejects_out_of_range_records(gpu, ctx8, oracle):
    """a record that indexes outside its dynamic dictionary is 'Invalid bitstream' (the reference's bounds-checked
    Matrix::operator[] throws), not a wild read."""
    import imageexperiments_amd as ia
    K, W, H = 8, 16, 8
    counts = np.zeros((2, 3), np.uint16)
    choices = np.zeros((2, 3, K), np.uint32)
    counts[0, 0] = 1
    choices[0, 0, 0] = 600 | (2 << 16)            # step 0 picks index 600 although only 510 base atoms exist
    blob = ia.assemble_streams(W, H, K, 8, ctx8.quant, counts, choices)
    with pytest.raises(ia.MpcError) as e:
        ia.decode_image(blob, ctx8)
    assert e.value.status == ia.api.MPC_ERR_BITSTREAM


def test_multi_batch_path_equals_single_batch(gpu, oracle, monkeypatch):
    """Inputs larger than the in-flight limit are processed as several sub-batches on the internal streams (the 8K
    config does this for real); forced here with a 256-tile limit on a 2000-tile frame and checked against the oracle."""
    import imageexperiments_amd as ia
    monkeypatch.setenv("MPC_MAX_BATCH_TILES", "256")
    monkeypatch.setenv("MPC_PIPES", "3")
    rgb = oracle.synth_frame(400, 320, 77)            # 50 x 40 tiles -> 8 sub-batches over 3 pipes
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    octx = oracle.OracleContext(8, 8, 3.5)
    _compare(ctx.encode_tiles(rgb), octx.encode_tiles(rgb), 8)
    ctx.close()


@pytest.mark.parametrize("workload", ["raise", "8k"])
def test_full_size_big_frames_sampled_against_oracle(gpu, oracle, workload):
    """BASELINE configs 3 and 5 at full size (4928x3264 K=32, 7680x4320 K=16; quality 3.5): tile columns sampled
    across the frame equal the oracle exactly; all records are self-consistent (swept rows follow from records)."""
    import bench
    import imageexperiments_amd as ia
    W, H, K, q = bench.WORKLOADS[workload]
    rgb = bench.synth_frame(W, H, 12345)
    ctx = ia.create_compression_context(K, 8, q, device=0)
    counts, choices, energy, swept = ctx.encode_tiles(rgb)
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    assert counts.shape[0] == tiles_x * tiles_y
    octx = oracle.OracleContext(K, 8, q)
    for tx in (0, tiles_x // 2 + 3, tiles_x - 1):
        oc, od, ok, oe, os_ = octx.encode_tiles(rgb, tx_begin=tx, tx_end=tx + 1)
        sl = slice(tx * tiles_y, (tx + 1) * tiles_y)
        assert (counts[sl] == oc[sl]).all()
        valid = np.arange(K)[None, None, :] <= np.minimum(oc[sl][:, :, None], K - 1)
        assert (choices["deltaId"][sl][valid] == od[sl][valid]).all()
        assert (choices["intCoeff"][sl][valid] == ok[sl][valid]).all()
        assert (swept[sl] == os_[sl]).all()
        assert (energy[sl].view(np.uint64) == oe[sl].view(np.uint64)).all()
    assert counts.max() <= K
    ctx.close()


@pytest.mark.parametrize("bpp", [2.0, 2.5, 3.0, 4.0, 5.0, 6.0])
def test_quality_sweep_on_a_crop_bytes_equal_oracle(gpu, oracle, bpp):
    """BASELINE config 3 sweeps quality 2.0 .. 6.0: whole-container byte identity on a 256x192 crop per quality."""
    import bench
    import imageexperiments_amd as ia
    rgb = np.ascontiguousarray(bench.synth_frame(4928, 3264, 12345)[1000:1192, 2000:2256])
    ctx = ia.create_compression_context(32, 8, bpp, device=0)
    assert ctx.encode_image(rgb) == oracle.OracleContext(32, 8, bpp).encode_image(rgb)
    ctx.close()


# ---- the MFMA filter: records must not depend on it ------------------------------------------------------------------

@pytest.mark.parametrize("channel", [0, 2])
def test_filter_adversarial_vectors_bit_exact(ctx32, octx32, channel):
    v = _adversarial_vectors()
    v = v[np.abs(v).max(axis=1) < 1e6]          # beyond that round(p / q) leaves the int range in the reference (UB there)
    counts, choices, energy, swept = ctx32.calc_mp(channel, v)
    for i in range(v.shape[0]):
        cnt, d, k, res, S = octx32.calc_mp(channel, v[i])
        assert counts[i] == cnt, i
        n = min(cnt + 1, 32)
        assert (choices["deltaId"][i, :n] == d[:n]).all(), i
        assert (choices["intCoeff"][i, :n] == k[:n]).all(), i
        assert swept[i] == S, i


def test_filter_adversarial_vectors_tiny_quant(ctx32, octx32):
    """a quantisation step far below the data keeps every pursuit alive for all 32 steps, whatever the magnitude: the
    filter sees residuals shrinking towards rounding noise with deep block lists"""
    v = _adversarial_vectors()
    v = v[np.abs(v).max(axis=1) < 1e100]                       # round(p / q) must stay inside int range in the reference too
    scale = np.maximum(np.abs(v).max(axis=1), 1e-290)
    for i in range(0, v.shape[0], 16):
        vv = v[i:i + 16]
        for j in range(vv.shape[0]):
            q = np.full(32, scale[i + j] * 2.0 ** -20)
            counts, choices, energy, swept = ctx32.calc_mp(0, vv[j:j + 1], quant_k=q)
            cnt, d, k, res, S = octx32.calc_mp(0, vv[j], quant=q)
            assert counts[0] == cnt, (i + j)
            n = min(cnt + 1, 32)
            assert (choices["deltaId"][0, :n] == d[:n]).all(), (i + j)
            assert (choices["intCoeff"][0, :n] == k[:n]).all(), (i + j)
            assert swept[0] == S


def test_filter_equals_exact_sweep_on_a_whole_frame(gpu, oracle, monkeypatch):
    """the product's own exhaustive sweep (every row correlated in double, MPC_FILTER=0) and the filtered path must
    agree on every record of a 1080p frame and of a K=32 frame -- 100 000+ pursuits, no sampling"""
    import imageexperiments_amd as ia
    for (w, h, K, seed) in ((1920, 1080, 8, 4242), (640, 480, 32, 99)):
        rgb = oracle.synth_frame(w, h, seed)
        ctx = ia.create_compression_context(K, 8, 3.5, device=0)
        monkeypatch.setenv("MPC_FILTER", "1")
        a = ctx.encode_tiles(rgb)
        monkeypatch.setenv("MPC_FILTER", "0")
        b = ctx.encode_tiles(rgb)
        monkeypatch.delenv("MPC_FILTER")
        ctx.close()
        assert (a[0] == b[0]).all()
        assert (a[1]["deltaId"] == b[1]["deltaId"]).all() and (a[1]["intCoeff"] == b[1]["intCoeff"]).all()
        assert (a[2].view(np.uint64) == b[2].view(np.uint64)).all()
        assert (a[3] == b[3]).all()


def test_pipelined_frames_equal_single_frame_calls(gpu, oracle):
    """mpc_encode_images overlaps the host entropy stage with the next frame's device encode: same bytes, frame by frame"""
    import imageexperiments_amd as ia
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    frames = [oracle.synth_frame(320, 200, 500 + f) for f in range(5)]
    singles = [bytes(ctx.encode_image(f)) for f in frames]
    batch = [bytes(b) for b in ctx.encode_images(frames)]
    assert batch == singles
    octx = oracle.OracleContext(8, 8, 3.5)
    assert batch[3] == bytes(octx.encode_image(frames[3]))
    # more frames than slots, then a larger and a smaller geometry on the same context (staging regrows), then one frame
    for (w, h, n) in ((320, 200, 11), (500, 333, 6), (64, 40, 9), (64, 40, 1)):
        frames = [oracle.synth_frame(w, h, 900 + 7 * f) for f in range(n)]
        assert [bytes(b) for b in ctx.encode_images(frames)] == [bytes(ctx.encode_image(f)) for f in frames], (w, h, n)
    ctx.close()


def test_natural_image_crops_bytes_equal_oracle(gpu, oracle, ctx32, octx32, mn_bytes):
    """natural content (crops of the reference's own photograph, decoded from its .mn fixture): the filter sees real
    edges, textures and flat sky instead of synthetic gradients; bytes must equal the oracle's"""
    import imageexperiments_amd as ia
    photo = ia.decode_image(mn_bytes, ctx32)
    for (x0, y0, w, h) in ((1000, 800, 256, 192), (3000, 2000, 320, 160), (0, 0, 200, 120), (4600, 3100, 328, 164)):
        crop = np.ascontiguousarray(photo[y0:y0 + h, x0:x0 + w])
        assert bytes(ctx32.encode_image(crop)) == bytes(octx32.encode_image(crop)), (x0, y0)


@pytest.mark.parametrize("env", [{"MPC_PATH": "steps"}, {"MPC_PIPES": "1"}, {"MPC_PIPES": "4"}, {"MPC_FILTER": "0"}])
def test_launch_configurations_do_not_change_records(gpu, oracle, monkeypatch, env):
    """the exhaustive sweep under both of its switch names, other sub-batch counts: same records"""
    import imageexperiments_amd as ia
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rgb = oracle.synth_frame(328, 208, 321)
    ctx = ia.create_compression_context(16, 8, 3.0, device=0)
    octx = oracle.OracleContext(16, 8, 3.0)
    _compare(ctx.encode_tiles(rgb), octx.encode_tiles(rgb), 16)
    ctx.close()


@pytest.mark.parametrize("workgroups", [1, 7, 224, 0])
def test_workgroup_limit_does_not_change_records(gpu, oracle, workgroups):
    """mpc_context_set_tile_encode_workgroups: the tile encode on fewer CUs (what a frame sequence and the multi-GPU drivers do
    to leave room for the kernels behind it) finds the same records; 0 gives all CUs back"""
    import imageexperiments_amd as ia
    rgb = oracle.synth_frame(328, 208, 77)
    ctx = ia.create_compression_context(16, 8, 3.0, device=0)
    octx = oracle.OracleContext(16, 8, 3.0)
    ctx.set_tile_encode_workgroups(workgroups)
    _compare(ctx.encode_tiles(rgb), octx.encode_tiles(rgb), 16)
    assert bytes(ctx.encode_image(rgb)) == bytes(octx.encode_image(rgb))
    with pytest.raises(ia.MpcError):
        ctx.set_tile_encode_workgroups(-1)
    ctx.close()


@pytest.mark.parametrize("stripes", [2, 3, 4])
def test_single_host_frame_in_row_stripes_bytes_equal_oracle(gpu, oracle, monkeypatch, stripes):
    """mpc_encode_image from host memory uploads and encodes a large frame in row stripes (each stripe's tile encode behind its own
    copy, records written in whole-frame order); forced here on small frames, ragged edges included"""
    import imageexperiments_amd as ia
    monkeypatch.setenv("MPC_SINGLE_STRIPES", str(stripes))
    ctx = ia.create_compression_context(16, 8, 3.0, device=0)
    octx = oracle.OracleContext(16, 8, 3.0)
    for (w, h, seed) in ((328, 208, 5), (203, 517, 6), (64, 136, 7)):
        rgb = oracle.synth_frame(w, h, seed)
        assert bytes(ctx.encode_image(rgb)) == bytes(octx.encode_image(rgb)), (w, h, stripes)
    ctx.close()


@pytest.mark.parametrize("K", [1, 8, 32])
def test_degenerate_frames_bytes_equal_oracle(gpu, oracle, K):
    """Flat frames (black: every residual is zero from the start; white and grey: only the DC atom matters), one-pixel
    checkerboards and stripes (energy in the highest frequencies), hard 0/255 noise and a 1x1 image, for the smallest
    and the largest K: container bytes equal the oracle's and decode to the oracle's pixels."""
    import imageexperiments_amd as ia
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    octx = oracle.OracleContext(K, 8, 3.5)
    frames = degenerate_frames(K)
    for name, rgb in frames.items():
        blob, ref = ctx.encode_image(rgb), octx.encode_image(rgb)
        assert blob == ref, name
        assert (ia.decode_image(blob, ctx) == oracle.decode_image(ref)).all(), name
    ctx.close()


@pytest.mark.parametrize("world,rank", [(2, 0), (2, 1), (4, 2), (8, 7)])
def test_batch_stripe_launch_equals_oracle(gpu, oracle, world, rank):
    """What one rank does per step in `bench.py --gpus N`: stripe `rank` of `world` frames in ONE launch of
    mpc_encode_batch_device, output tile index = frame * tiles_per_stripe + tx * rows + (ty - row_begin).  Checked
    against the oracle's whole-frame records of every frame, restricted to the stripe."""
    import imageexperiments_amd as ia
    from imageexperiments_amd.sharding import stripe_bounds
    torch = gpu
    K, W, H = 8, 136, 100                                    # 17 whole tile columns (3 W % 8 == 0), 13 tile rows, the last ragged;
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8            # a ragged width in a batch: test_gpu_frame_layouts.py, batch-ragged
    r0, r1 = stripe_bounds(tiles_y, world, rank)
    rows = r1 - r0
    frames = world
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    octx = oracle.OracleContext(K, 8, 3.5)
    host = np.stack([oracle.synth_frame(W, H, 40 + f) for f in range(frames)])
    d_rgb = torch.from_numpy(host).cuda()
    tiles = frames * tiles_x * rows
    d_counts = torch.zeros((max(tiles, 1), 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((max(tiles, 1), 3, K), dtype=torch.int32, device="cuda")
    if rows > 0:
        ctx.encode_batch_device(d_rgb.data_ptr(), frames, W * H * 3, W, H, W * 3, r0, r1, d_counts.data_ptr(), d_choices.data_ptr())
        torch.cuda.synchronize()
    counts = d_counts.cpu().numpy().view(np.uint16)[:tiles].reshape(frames, tiles_x, rows, 3)
    choices = d_choices.cpu().numpy().view(np.uint32)[:tiles].reshape(frames, tiles_x, rows, 3, K)
    for f in range(frames):
        oc, od, ok, _, _ = octx.encode_tiles(host[f])
        oc = oc.reshape(tiles_x, tiles_y, 3)[:, r0:r1]
        orec = (od.astype(np.uint32) | (ok.astype(np.uint32) << 16)).reshape(tiles_x, tiles_y, 3, K)[:, r0:r1]
        assert (counts[f] == oc).all(), f
        live = np.arange(K)[None, None, None, :] < np.minimum(oc.astype(np.int64) + 1, K)[..., None]   # records 0..count
        assert (choices[f][live] == orec[live]).all(), f
    ctx.close()


def test_nan_vectors_end_the_pursuit_like_the_reference(ctx32, octx32):
    """A NaN anywhere in the input makes every projection NaN; `abs(p) > best` is false for all rows, Select returns -1
    and CalcMPDynamic returns 0 (MatchingPursuit.cpp:50-54).  The filter must not lose that: NaN approximations keep
    every row as a survivor and the exact evaluations decide.  (Infinities are left out: round(inf / q) -> int is
    undefined behaviour in the reference.)"""
    v = nan_vectors()
    for channel in (0, 1):
        counts, choices, energy, swept = ctx32.calc_mp(channel, v)
        for i in range(v.shape[0]):
            cnt, d, k, res, S = octx32.calc_mp(channel, v[i])
            assert counts[i] == cnt, i
            n = min(cnt + 1, 32) if i >= 5 else 0
            assert (choices["deltaId"][i, :n] == d[:n]).all(), i
            assert (choices["intCoeff"][i, :n] == k[:n]).all(), i
            assert swept[i] == S, i
        assert (counts[:5] == 0).all()


def test_many_near_ties_on_one_lane(ctx32, octx32):
    """ADVICE r1 (survivor queue): residuals built as equal-weight sums of several base rows give a tile-channel three or
    more rows inside the filter window at once, next to clear neighbours in the same column group."""
    base, rows, det = ctx32.dictionary()
    v = near_tie_vectors(base)
    counts, choices, energy, swept = ctx32.calc_mp(0, v)
    for i in range(v.shape[0]):
        cnt, d, k, res, S = octx32.calc_mp(0, v[i])
        assert counts[i] == cnt, i
        n = min(cnt + 1, 32)
        assert (choices["deltaId"][i, :n] == d[:n]).all(), i
        assert (choices["intCoeff"][i, :n] == k[:n]).all(), i
        assert swept[i] == S, i


def test_quant_override_does_not_stick(ctx32, octx32, oracle):
    """a per-call quantiser table must not replace the context's device table.  Encode with an
    override (explicitly, and through the patch statistics, which quantise with all ones), then with quant=None:
    the container must be the oracle's for the context's own tables."""
    import imageexperiments_amd as ia
    rgb = oracle.synth_frame(104, 72, 31)
    want = bytes(octx32.encode_image(rgb))
    assert bytes(ctx32.encode_image(rgb)) == want
    ones = np.ones((3, 32))
    ctx32.encode_tiles(rgb, quant=ones)
    assert bytes(ctx32.encode_image(rgb)) == want
    ps = ia.api.PatchStatistics(ctx32, 7)
    ps.add_image(rgb, 32)
    ps.close()
    assert bytes(ctx32.encode_image(rgb)) == want
    custom = octx32.quant * 2.0
    assert bytes(ctx32.encode_image(rgb, quant=custom)) == bytes(octx32.encode_image(rgb, quant=custom))
    assert bytes(ctx32.encode_image(rgb)) == want
    # decode side: an override on mpc_decode_tiles_device must not stick either
    back = ia.api.decode_image(want, ctx32)
    assert (back == oracle.decode_image(want)).all()


def test_device_resident_frames_to_containers(gpu, oracle):
    """mpc_encode_image(s)_device: frames already in HBM -> tile encode + stream assembly on the device -> host entropy stage.
    Same bytes as the oracle's encodeImage, for several K (record alignment), ragged sizes and more frames than slots."""
    import imageexperiments_amd as ia
    for (w, h, K, q, n) in ((200, 136, 32, 3.5, 6), (129, 77, 8, 3.5, 3), (64, 64, 5, 2.0, 2), (1003, 517, 16, 4.0, 1)):
        ctx = ia.create_compression_context(K, 8, q, device=0)
        octx = oracle.OracleContext(K, 8, q)
        frames = [oracle.synth_frame(w, h, 40 + f) for f in range(n)]
        d = [gpu.from_numpy(f).cuda() for f in frames]
        blobs = ctx.encode_images_device([t.data_ptr() for t in d], w, h)
        for f in range(n):
            assert bytes(blobs[f]) == bytes(octx.encode_image(frames[f])), (w, h, K, f)
        assert bytes(ctx.encode_image_device(d[0].data_ptr(), w, h)) == bytes(blobs[0])
        ctx.close()


def test_container_job_survives_other_calls_on_its_context(gpu, oracle):
    """A container job owns its buffers: between `begin` and `collect` the context may encode other frames (other geometry: the
    frame pipeline re-carves and clears ITS entropy slots), decode, and run a second job -- every container still equals the
    oracle's (the job used to share the pipeline's slot buffers)."""
    import torch
    import imageexperiments_amd as ia
    K = 16
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    octx = oracle.OracleContext(K, 8, 3.5)
    W, H = 136, 104
    rgb = oracle.synth_frame(W, H, 77)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    d_rgb = torch.from_numpy(rgb).cuda()
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, (H + 7) // 8, d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    want = bytes(octx.encode_image(rgb))
    other = oracle.synth_frame(200, 72, 5)                                   # another geometry through the same context
    want_other = bytes(octx.encode_image(other))
    ctx.container_job_begin(0, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    assert bytes(ctx.encode_image(other)) == want_other                    # between begin and tables
    ctx.container_job_begin(1, d_counts.data_ptr(), d_choices.data_ptr(), W, H)     # a second job on the same records
    ctx.container_job_tables(0)
    blobs = ctx.encode_images([other, other, other])                        # between tables and collect: the pipeline's slots
    assert [bytes(b) for b in blobs] == [want_other] * 3
    assert [bytes(b) for b in ctx.encode_images([rgb, rgb])] == [want] * 2  # ... and the job's own geometry
    assert (ia.api.decode_image(want_other, ctx) == oracle.decode_image(want_other)).all()
    ctx.container_job_tables(1)
    assert bytes(ctx.container_job_collect(0)) == want
    assert bytes(ctx.container_job_collect(1)) == want
    assert bytes(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), W, H)) == want
    # a job given up half way leaves its slot usable
    ctx.container_job_begin(2, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    with pytest.raises(ia.MpcError):
        ctx.container_job_begin(2, d_counts.data_ptr(), d_choices.data_ptr(), W, H)        # busy
    ctx.container_job_cancel(2)
    ctx.container_job_begin(2, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    ctx.container_job_tables(2)
    ctx.container_job_cancel(2)
    ctx.container_job_begin(2, d_counts.data_ptr(), d_choices.data_ptr(), W, H)
    ctx.container_job_tables(2)
    assert bytes(ctx.container_job_collect(2)) == want
