"""The float pursuit kernel (`mp_pursuit_kernel<float, 12>`, behind mpc_context_set_fast) held to the double kernel's parity tests
(run with -m gpu): every test of test_gpu_parity.py that the float flavour lacked, same shapes and seeds, against
OracleFastContext (oracle/mpo_fast.c).  Everything is bit equality: counts, records 0..count INCLUSIVE (the terminating record
too), swept rows, the float residual energy, container bytes, and decoded pixels against oracle.decode_image_fast.

The vector inputs come from tests/pursuit_cases.py, in two forms (the context's tables / the tiny step); tests/test_pursuit_cases.py
proves on the CPU that they are well defined in the float oracle and that the tiny form tells float arithmetic from double
arithmetic.  The last tests hold BOTH flavours to what include/mpcodec.h promises about the output buffers."""
import numpy as np
import pytest

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
def fast32(ia):
    return ia.create_compression_context(32, 8, 3.5, device=0).set_fast(True)


@pytest.fixture(scope="module")
def ofast32(oracle, octx32):
    return oracle.OracleFastContext(octx32)


@pytest.fixture(scope="module")
def classes(octx32):
    return pc.float_cases(octx32.base, octx32.det_rows, octx32.det[0])


def _fast_pair(ia, oracle, K, bpp):
    ctx = ia.create_compression_context(K, 8, bpp, device=0).set_fast(True)
    return ctx, oracle.OracleFastContext(oracle.OracleContext(K, 8, bpp))


def _compare(gpu_out, ora_out, K):
    counts, choices, energy, swept = gpu_out
    ocounts, odelta, ocoef, oenergy, oswept = ora_out
    assert (counts == ocounts).all(), f"{(counts != ocounts).sum()} count mismatches"
    valid = np.arange(K)[None, None, :] <= np.minimum(ocounts[:, :, None], K - 1)      # records 0..count inclusive
    assert (choices["deltaId"][valid] == odelta[valid]).all()
    assert (choices["intCoeff"][valid] == ocoef[valid]).all()
    assert (swept == oswept).all()
    assert (energy.view(np.uint64) == oenergy.view(np.uint64)).all(), "energy not bit-identical"


def _check_one(got, want, i, K, what):
    """one vector: device outputs row i against an OracleFastContext.calc_mp result"""
    counts, choices, energy, swept = got
    cnt, d, k, res, S = want
    assert counts[i] == cnt, (what, int(counts[i]), cnt)
    n = min(cnt + 1, K)                                                  # records 0..count inclusive
    assert (choices["deltaId"][i, :n] == d[:n]).all(), what
    assert (choices["intCoeff"][i, :n] == k[:n]).all(), what
    assert swept[i] == S, what
    e = pc.f32_energy(res)
    if np.isfinite(e):                                                   # compared where the oracle's float sum is finite
        assert energy[i] == e, what


def _check_class(ctx, of, channel, kept, form, name):
    K = ctx.K
    if form == "table":
        got = ctx.calc_mp(channel, kept)
        for i in range(kept.shape[0]):
            _check_one(got, of.calc_mp(channel, kept[i]), i, K, (name, form, channel, i))
    else:
        for i in range(kept.shape[0]):
            q = pc.tiny_quant(kept[i], K)
            _check_one(ctx.calc_mp(channel, kept[i:i + 1], quant_k=q), of.calc_mp(channel, kept[i], quant=q), 0, K,
                       (name, form, channel, i))


CLASS_NAMES = ["adversarial", "near_ties_base", "near_ties_detail", "nan", "f32_subnormal_inputs", "f32_subnormal_products",
               "f32_subnormal_residuals", "f32_large", "zero_and_sign"]


@pytest.mark.parametrize("channel", [0, 2])
@pytest.mark.parametrize("name", [n for n in CLASS_NAMES if "table" in pc.forms_of(n)])      # f32_large: tiny step only
def test_vector_classes_with_the_context_tables(fast32, ofast32, classes, name, channel):
    """test_filter_adversarial_vectors_bit_exact, test_many_near_ties_on_one_lane and the float-only classes: the screen's
    thresholds with the quantiser tables a frame sees.  (The two oracles agree on all of these, see test_pursuit_cases.py;
    the tiny form below is what tells the arithmetic apart.)"""
    kept, _ = classes[(name, "table")]
    _check_class(fast32, ofast32, channel, kept, "table", name)


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_vector_classes_with_the_tiny_step(fast32, ofast32, classes, name):
    """test_filter_adversarial_vectors_tiny_quant on every class: q = max(max|v| * 2^-20, 2^-126) keeps the pursuit alive for
    all 32 steps where the data allow it (counts in test_pursuit_cases.py).  f32 range edges: subnormal inputs, subnormal
    products, residuals that become subnormal after some steps -- the oracle is built without fast-math and keeps subnormals,
    so a kernel that flushed them would differ -- and magnitudes up to 1e37, the largest that overflow nothing."""
    kept, _ = classes[(name, "tiny")]
    _check_class(fast32, ofast32, 0, kept, "tiny", name)


def test_nan_vectors_end_the_pursuit_like_the_float_oracle(fast32, ofast32):
    """What the float oracle does with a NaN: every projection is a sum over all 64 elements, so one NaN makes every projection
    NaN; index -1 needs `fabsf(p) > best_abs` (best_abs = -1) false for EVERY row, which is exactly that; the pursuit returns
    count 0 with record (0, 0) and 510 rows swept.  The screen must keep every row a survivor so that the exact chain decides."""
    v = pc.nan_vectors()
    for channel in (0, 1):
        got = fast32.calc_mp(channel, v)
        for i in range(v.shape[0]):
            _check_one(got, ofast32.calc_mp(channel, v[i]), i, 32, ("nan", channel, i))
        counts, choices, _, swept = got
        assert (counts[:pc.NAN_ROWS] == 0).all() and (counts[pc.NAN_ROWS:] > 0).all()
        assert (choices["deltaId"][:pc.NAN_ROWS, 0] == 0).all() and (choices["intCoeff"][:pc.NAN_ROWS, 0] == 0).all()
        assert (swept[:pc.NAN_ROWS] == 510).all()


def test_zero_vector_selects_row_zero_with_coefficient_zero(fast32, ofast32, octx32):
    """`best_abs` starts at -1 (Eigen's maxCoeff): an all-zero (or all negative-zero) vector chooses row 0, quantises to 0 and
    ends with count 0, record (0, 0); a vector orthogonal to row 0 goes on to the row that really is the largest."""
    z = pc.as_f32(pc.zero_and_sign_vectors(octx32.base))
    counts, choices, energy, swept = fast32.calc_mp(0, z)
    assert (counts[:2] == 0).all() and (choices["deltaId"][:2, 0] == 0).all() and (choices["intCoeff"][:2, 0] == 0).all()
    assert (swept[:2] == 510).all() and (energy[:2] == 0).all()
    for i in range(2, 14):
        q = pc.tiny_quant(z[i], 32)
        c, r, _, _ = fast32.calc_mp(0, z[i:i + 1], quant_k=q)
        assert c[0] > 0 and r["deltaId"][0, 0] != 0


@pytest.mark.parametrize("workgroups", [1, 7, 224, 0])
def test_workgroup_limit_does_not_change_records(ia, oracle, workgroups):
    """one workgroup makes its twelve waves walk all three channels and hand the home tiles over twice"""
    rgb = oracle.synth_frame(328, 208, 77)
    ctx, of = _fast_pair(ia, oracle, 16, 3.0)
    ctx.set_tile_encode_workgroups(workgroups)
    _compare(ctx.encode_tiles(rgb), of.encode_tiles(rgb), 16)
    assert bytes(ctx.encode_image(rgb)) == bytes(of.encode_image(rgb))
    q = pc.fine_table(16)                                    # the table with which every tile row shows its flavour
    _compare(ctx.encode_tiles(rgb, quant=q), of.encode_tiles(rgb, quant=q), 16)
    assert bytes(ctx.encode_image(rgb, quant=q)) == bytes(of.encode_image(rgb, quant=q))
    ctx.close()


def test_row_stripes_equal_full_frame(fast32, ofast32, oracle):
    rgb = oracle.synth_frame(80, 72, 4242)       # 10 x 9 tiles
    full = fast32.encode_tiles(rgb)
    _compare(full, ofast32.encode_tiles(rgb), 32)
    tx, ty = 10, 9
    for a, b in ((0, 4), (4, 9), (8, 9)):
        part = fast32.encode_tiles(rgb, a, b)
        rows = b - a
        for arr_full, arr_part in zip(full, part):
            f = arr_full.reshape((tx, ty) + arr_full.shape[1:])[:, a:b]
            assert (f.reshape((tx * rows,) + arr_full.shape[1:]) == arr_part).all()


@pytest.mark.parametrize("stripes", [2, 3, 4])
def test_single_host_frame_in_row_stripes_bytes_equal_oracle(ia, oracle, monkeypatch, stripes):
    monkeypatch.setenv("MPC_SINGLE_STRIPES", str(stripes))
    ctx, of = _fast_pair(ia, oracle, 16, 3.0)
    for (w, h, seed) in ((328, 208, 5), (203, 517, 6), (64, 136, 7)):
        rgb = oracle.synth_frame(w, h, seed)
        assert bytes(ctx.encode_image(rgb)) == bytes(of.encode_image(rgb)), (w, h, stripes)
    ctx.close()


@pytest.mark.parametrize("world,rank", [(2, 0), (2, 1), (4, 2), (8, 7)])
def test_batch_stripe_launch_equals_oracle(ia, oracle, world, rank):
    import torch
    from imageexperiments_amd.sharding import stripe_bounds
    K, W, H = 8, 136, 100                                    # 17 x 13 tiles, ragged in both directions
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    r0, r1 = stripe_bounds(tiles_y, world, rank)
    rows = r1 - r0
    frames = world
    ctx, of = _fast_pair(ia, oracle, K, 3.5)
    host = np.stack([oracle.synth_frame(W, H, 40 + f) for f in range(frames)])
    d_rgb = torch.from_numpy(host).cuda()
    tiles = frames * tiles_x * rows
    for q in (None, pc.fine_table(K)):                       # the context's tables; the table that shows the flavour
        d_counts = torch.zeros((max(tiles, 1), 3), dtype=torch.int16, device="cuda")
        d_choices = torch.zeros((max(tiles, 1), 3, K), dtype=torch.int32, device="cuda")
        if rows > 0:
            ctx.encode_batch_device(d_rgb.data_ptr(), frames, W * H * 3, W, H, W * 3, r0, r1, d_counts.data_ptr(), d_choices.data_ptr(),
                                    quant=q)
            torch.cuda.synchronize()
        counts = d_counts.cpu().numpy().view(np.uint16)[:tiles].reshape(frames, tiles_x, rows, 3)
        choices = d_choices.cpu().numpy().view(np.uint32)[:tiles].reshape(frames, tiles_x, rows, 3, K)
        for f in range(frames):
            oc, od, ok, _, _ = of.encode_tiles(host[f], quant=q)
            oc = oc.reshape(tiles_x, tiles_y, 3)[:, r0:r1]
            orec = (od.astype(np.uint32) | (ok.astype(np.uint32) << 16)).reshape(tiles_x, tiles_y, 3, K)[:, r0:r1]
            assert (counts[f] == oc).all(), (f, q is None)
            live = np.arange(K)[None, None, None, :] < np.minimum(oc.astype(np.int64) + 1, K)[..., None]   # records 0..count
            assert (choices[f][live] == orec[live]).all(), (f, q is None)
    ctx.close()


def test_pipelined_frames_equal_single_frame_calls(ia, oracle):
    ctx, of = _fast_pair(ia, oracle, 8, 3.5)
    frames = [oracle.synth_frame(320, 200, 500 + f) for f in range(5)]
    singles = [bytes(ctx.encode_image(f)) for f in frames]
    batch = [bytes(b) for b in ctx.encode_images(frames)]
    assert batch == singles
    assert batch[3] == bytes(of.encode_image(frames[3]))
    # more frames than slots, then a larger and a smaller geometry on the same context (staging regrows), then one frame
    for (w, h, n) in ((320, 200, 11), (500, 333, 6), (64, 40, 9), (64, 40, 1)):
        frames = [oracle.synth_frame(w, h, 900 + 7 * f) for f in range(n)]
        got = [bytes(b) for b in ctx.encode_images(frames)]
        assert got == [bytes(ctx.encode_image(f)) for f in frames], (w, h, n)
        assert got[n - 1] == bytes(of.encode_image(frames[n - 1])), (w, h, n)
    ctx.close()


def test_flavour_switches_between_calls_give_each_flavours_own_bytes(ia, oracle):
    """The frame pipeline's slots, the quantiser upload and the workspace are shared between the flavours: a context switched
    float -> double -> float between calls must give each flavour's own bytes every time, single frames and sequences."""
    K = 8
    ctx = ia.create_compression_context(K, 8, 3.5, device=0)
    octx = oracle.OracleContext(K, 8, 3.5)
    of = oracle.OracleFastContext(octx)
    frames = [oracle.synth_frame(320, 200, 700 + f) for f in range(7)]
    want = {True: [bytes(of.encode_image(f)) for f in frames], False: [bytes(octx.encode_image(f)) for f in frames]}
    assert want[True] != want[False]
    for fast in (True, False, True, False, True):
        ctx.set_fast(fast)
        assert ctx.fast == fast
        assert [bytes(b) for b in ctx.encode_images(frames)] == want[fast], fast
        assert bytes(ctx.encode_image(frames[2])) == want[fast][2], fast
        _compare(ctx.encode_tiles(frames[0]), (of if fast else octx).encode_tiles(frames[0]), K)
    ctx.close()


@pytest.mark.parametrize("K", [1, 8, 32])
def test_degenerate_frames_bytes_equal_oracle(ia, oracle, K):
    ctx, of = _fast_pair(ia, oracle, K, 3.5)
    for name, rgb in pc.degenerate_frames(K).items():
        blob, ref = ctx.encode_image(rgb), of.encode_image(rgb)
        assert blob == ref, name
        assert (ia.decode_image(blob, ctx) == oracle.decode_image_fast(ref)).all(), name
    ctx.close()


@pytest.mark.parametrize("bpp", [2.0, 2.5, 3.0, 4.0, 5.0, 6.0])
def test_quality_sweep_on_a_crop_bytes_equal_oracle(ia, oracle, bpp):
    import bench
    rgb = np.ascontiguousarray(bench.synth_frame(4928, 3264, 12345)[1000:1192, 2000:2256])
    ctx, of = _fast_pair(ia, oracle, 32, bpp)
    assert ctx.encode_image(rgb) == of.encode_image(rgb)
    ctx.close()


def test_natural_image_crops_bytes_equal_oracle(ia, oracle, fast32, ofast32, mn_bytes):
    """the crops of test_gpu_parity.py's test (the photograph decoded by the double decoder, so the pixels are the same)"""
    dctx = ia.create_compression_context(32, 8, 3.5, device=0)
    photo = ia.decode_image(mn_bytes, dctx)
    dctx.close()
    for (x0, y0, w, h) in ((1000, 800, 256, 192), (3000, 2000, 320, 160), (0, 0, 200, 120), (4600, 3100, 328, 164)):
        crop = np.ascontiguousarray(photo[y0:y0 + h, x0:x0 + w])
        blob = bytes(fast32.encode_image(crop))
        assert blob == bytes(ofast32.encode_image(crop)), (x0, y0)
        assert (ia.decode_image(blob, fast32) == oracle.decode_image_fast(blob)).all(), (x0, y0)


def test_quant_override_does_not_stick(ia, fast32, ofast32, oracle, octx32):
    rgb = oracle.synth_frame(104, 72, 31)
    want = bytes(ofast32.encode_image(rgb))
    assert bytes(fast32.encode_image(rgb)) == want
    ones = np.ones((3, 32))
    fast32.encode_tiles(rgb, quant=ones)
    assert bytes(fast32.encode_image(rgb)) == want
    ps = ia.api.PatchStatistics(fast32, 7)
    ps.add_image(rgb, 32)
    ps.close()
    assert bytes(fast32.encode_image(rgb)) == want
    custom = octx32.quant * 2.0
    assert bytes(fast32.encode_image(rgb, quant=custom)) == bytes(ofast32.encode_image(rgb, quant=custom))
    assert bytes(fast32.encode_image(rgb)) == want
    back = ia.api.decode_image(want, fast32)
    assert (back == oracle.decode_image_fast(want)).all()


# ---- both flavours: what include/mpcodec.h promises about the output buffers --------------------------------------------

@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("rows", [None, (3, 9)])
def test_dirty_output_buffers_records_then_zeros(ia, oracle, fast, rows):
    """`d_choices`: "records 0..count ...; entries beyond are zero".  The caller's buffers arrive filled with 0xFF bytes (Python's
    own wrapper always hands zeros): after mpc_encode_tiles_device every count, energy and swept entry is the oracle's, records
    0..count are the oracle's and EVERY entry beyond is zero -- full height and a stripe of a ragged frame; then
    mpc_records_to_container_device on the full-height records gives the oracle's bytes."""
    import torch
    K, W, H = 16, 203, 117                                   # 26 x 15 tiles, ragged in both directions
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    a, b = rows or (0, tiles_y)
    ctx = ia.create_compression_context(K, 8, 3.0, device=0).set_fast(fast)
    octx = oracle.OracleContext(K, 8, 3.0)
    o = oracle.OracleFastContext(octx) if fast else octx
    rgb = oracle.synth_frame(W, H, 99)
    tiles = tiles_x * (b - a)
    d_rgb = torch.from_numpy(rgb).cuda()
    dirty = lambda nbytes: torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")      # noqa: E731
    d_counts, d_choices, d_energy, d_swept = dirty(tiles * 3 * 2), dirty(tiles * 3 * K * 4), dirty(tiles * 3 * 8), dirty(tiles * 3 * 4)
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, a, b, d_counts.data_ptr(), d_choices.data_ptr(),
                            d_energy.data_ptr(), d_swept.data_ptr())
    torch.cuda.synchronize()
    _records_then_zeros(d_counts, d_choices, d_energy, d_swept, o.encode_tiles(rgb), 1, tiles_x, tiles_y, a, b, K)
    if rows is None:
        want = bytes(o.encode_image(rgb))
        assert bytes(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), W, H)) == want
    ctx.close()


@pytest.mark.parametrize("fast", [False, True])
def test_dirty_output_buffers_batch_launch(ia, oracle, fast):
    """the same for mpc_encode_batch_device: three frames, a stripe and the full height, buffers pre-filled with 0xFF"""
    import torch
    K, W, H = 8, 136, 100                                    # 17 x 13 tiles
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    ctx = ia.create_compression_context(K, 8, 3.5, device=0).set_fast(fast)
    octx = oracle.OracleContext(K, 8, 3.5)
    o = oracle.OracleFastContext(octx) if fast else octx
    frames = 3
    host = np.stack([oracle.synth_frame(W, H, 60 + f) for f in range(frames)])
    d_rgb = torch.from_numpy(host).cuda()
    want = [o.encode_tiles(host[f]) for f in range(frames)]
    for (a, b) in ((0, tiles_y), (5, 12)):
        tiles = frames * tiles_x * (b - a)
        dirty = lambda nbytes: torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")  # noqa: E731
        d_counts, d_choices, d_energy, d_swept = dirty(tiles * 3 * 2), dirty(tiles * 3 * K * 4), dirty(tiles * 3 * 8), dirty(tiles * 3 * 4)
        ctx.encode_batch_device(d_rgb.data_ptr(), frames, W * H * 3, W, H, W * 3, a, b, d_counts.data_ptr(), d_choices.data_ptr(),
                                d_energy.data_ptr(), d_swept.data_ptr())
        torch.cuda.synchronize()
        stacked = tuple(np.stack([w[i] for w in want]) for i in range(5))
        _records_then_zeros(d_counts, d_choices, d_energy, d_swept, stacked, frames, tiles_x, tiles_y, a, b, K)
    ctx.close()


def _records_then_zeros(d_counts, d_choices, d_energy, d_swept, want, frames, tiles_x, tiles_y, a, b, K):
    """device outputs of a stripe [a, b) (tile = frame, tx, ty - a) against whole-frame oracle outputs (tile = tx * tiles_y + ty)"""
    rows = b - a
    shape = (frames, tiles_x, rows, 3)
    counts = d_counts.cpu().numpy().view(np.uint16).reshape(shape)
    records = d_choices.cpu().numpy().view(np.uint32).reshape(shape + (K,))
    energy = d_energy.cpu().numpy().view(np.float64).reshape(shape)
    swept = d_swept.cpu().numpy().view(np.uint32).reshape(shape)
    oc, od, ok, oe, os_ = _stripe(want, frames, tiles_x, tiles_y, a, b, K)
    assert (counts == oc).all()
    orec = od.astype(np.uint32) | (ok.astype(np.uint32) << 16)
    step = np.arange(K)[None, None, None, None, :]
    live = step <= np.minimum(oc.astype(np.int64), K - 1)[..., None]                  # records 0..count
    assert (records[live] == orec[live]).all()
    assert (records[~live] == 0).all(), f"{int((records[~live] != 0).sum())} entries beyond the terminating record are not zero"
    assert (swept == os_).all()
    assert (energy.view(np.uint64) == oe.view(np.uint64)).all()


def _stripe(want, frames, tiles_x, tiles_y, a, b, K):
    oc, od, ok, oe, os_ = want
    oc = oc.reshape(frames, tiles_x, tiles_y, 3)[:, :, a:b]
    od = od.reshape(frames, tiles_x, tiles_y, 3, K)[:, :, a:b]
    ok = ok.reshape(frames, tiles_x, tiles_y, 3, K)[:, :, a:b]
    oe = np.ascontiguousarray(oe.reshape(frames, tiles_x, tiles_y, 3)[:, :, a:b])
    os_ = os_.reshape(frames, tiles_x, tiles_y, 3)[:, :, a:b]
    return oc, od, ok, oe, os_
