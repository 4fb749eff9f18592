"""Rate-distortion sweep on the device (run with -m gpu): mpc_rate_distortion[_device] and mpc_distortion_device.

For every level of a sweep: the container equals mpc_encode_image's with that table, the SSE equals numpy's exact sum against
decode_image(container), and the PSNR equals calculate_psnr bit for bit.  Double and fast contexts at K = 8 and 32."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LEVELS = [8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0, "max"]


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


_contexts = {}


def _context(ia, K, fast=False):
    key = (K, fast)
    if key not in _contexts:
        _contexts[key] = ia.create_compression_context(K, 8, 3.5, device=0).set_fast(fast)
    return _contexts[key]


@pytest.fixture(scope="module")
def photo(ia, mn_bytes):
    """The reference's own photograph (4928 x 3264), decoded from its .mn fixture by the product's decoder."""
    return np.ascontiguousarray(ia.decode_image(mn_bytes, _context(ia, 32)))


def _sse(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def _check_point(ia, ctx, rgb, p):
    blob = ctx.encode_image(rgb, quant=p.quant)
    assert p.container == blob, p
    assert p.size == len(blob)
    H, W = rgb.shape[:2]
    assert p.bpp == float(8 * len(blob)) / float(W * H)
    decoded = ia.decode_image(blob, ctx)
    assert p.sse == _sse(rgb, decoded), p
    ref = ia.calculate_psnr(rgb, decoded)
    assert np.float64(p.psnr).tobytes() == np.float64(ref).tobytes(), (p.psnr, ref)


def _synthetic(oracle, W, H, seed):
    return oracle.synth_frame(W, H, seed)


@pytest.mark.parametrize("K,fast", [(8, False), (32, False), (8, True), (32, True)])
def test_sweep_identities_on_ragged_frames(ia, oracle, photo, K, fast):
    ctx = _context(ia, K, fast)
    frames = [_synthetic(oracle, 203, 117, 11), _synthetic(oracle, 1, 1, 12), _synthetic(oracle, 9, 8, 13),
              np.ascontiguousarray(photo[1001:1001 + 77, 2003:2003 + 131]), np.ascontiguousarray(photo[:64, :72])]
    for rgb in frames:
        points = ctx.rate_distortion(rgb, LEVELS, keep_bytes=True)
        assert [p.quality for p in points] == LEVELS
        for p in points:
            _check_point(ia, ctx, rgb, p)
        sizes_only = ctx.rate_distortion(rgb, LEVELS)
        assert [(p.size, p.sse, p.psnr) for p in sizes_only] == [(p.size, p.sse, p.psnr) for p in points]
        assert all(p.container is None for p in sizes_only)


@pytest.mark.parametrize("K", [8, 32])
def test_sweep_matches_the_oracle_codec(ia, oracle, photo, K):
    ctx = _context(ia, K)
    octx = oracle.OracleContext(K, 8, 3.5)
    rgb = np.ascontiguousarray(photo[2000:2048, 1500:1564])              # 64 x 48
    for p in ctx.rate_distortion(rgb, [8.0, 3.5, 1.0, "max"], keep_bytes=True):
        blob = octx.encode_image(rgb, quant=p.quant)
        assert p.container == blob, p
        decoded = oracle.decode_image(blob)
        assert p.sse == _sse(rgb, decoded)
        assert np.float64(p.psnr).tobytes() == np.float64(ia.calculate_psnr(rgb, decoded)).tobytes()


def _device_records(ia, ctx, rgb, quant):
    import torch
    counts, choices, _e, _s = ctx.encode_tiles(rgb, quant=quant)
    d_counts = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
    d_choices = torch.from_numpy(np.ascontiguousarray(choices).view(np.uint32)).cuda()
    d_rgb = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    return d_counts, d_choices, d_rgb


def _decode_tiles(ia, ctx, d_counts, d_choices, quant, W, H):
    import torch
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    q = np.ascontiguousarray(quant, np.float64)
    st = ctx.L.mpc_decode_tiles_device(ctx.h, d_counts.data_ptr(), d_choices.data_ptr(), q.ctypes.data_as(C.POINTER(C.c_double)),
                                       W, H, out.data_ptr(), None)
    assert st == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("K,fast", [(8, False), (32, False), (8, True), (32, True)])
def test_non_integer_table_uses_the_header_values(ia, oracle, K, fast):
    ctx = _context(ia, K, fast)
    rgb = _synthetic(oracle, 203, 117, 21)
    table = ia.quant_tables(K, 3.5) * 1.37
    assert (table != np.floor(table)).any()
    (p,) = ctx.rate_distortion(rgb, [table], keep_bytes=True)
    assert p.quality == "table"
    _check_point(ia, ctx, rgb, p)
    assert np.array_equal(ia.read_compressed(p.container)["quant"], table.astype(np.uint16))
    # the same records reconstructed with the encoder's doubles would give another error: the truncation is what is pinned
    d_counts, d_choices, _ = _device_records(ia, ctx, rgb, table)
    with_doubles = _decode_tiles(ia, ctx, d_counts, d_choices, table, 203, 117)
    with_header = _decode_tiles(ia, ctx, d_counts, d_choices, np.floor(table), 203, 117)
    assert p.sse == _sse(rgb, with_header)
    assert p.sse != _sse(rgb, with_doubles)


def test_all_zero_frame_is_lossless(ia):
    ctx = _context(ia, 8)
    rgb = np.zeros((24, 40, 3), np.uint8)
    for p in ctx.rate_distortion(rgb, [8.0, 1.0, "max"], keep_bytes=True):
        assert p.sse == 0
        assert p.psnr == float("inf")
        decoded = ia.decode_image(p.container, ctx)
        assert ia.calculate_psnr(rgb, decoded) == float("inf")


@pytest.mark.parametrize("K,fast", [(8, False), (32, False), (8, True), (32, True)])
def test_tile_sums_in_reference_order(ia, oracle, K, fast):
    import torch
    ctx = _context(ia, K, fast)
    W, H = 203, 117
    rgb = _synthetic(oracle, W, H, 31)
    quant = ia.quant_tables(K, 2.0)
    d_counts, d_choices, d_rgb = _device_records(ia, ctx, rgb, quant)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    d_sse = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_tiles = torch.zeros(tx * ty, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.distortion_device(d_counts.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), W, H, d_sse.data_ptr(), d_tiles.data_ptr(),
                          quant=quant)
    torch.cuda.synchronize()
    tiles = d_tiles.cpu().numpy().view(np.uint32)
    decoded = _decode_tiles(ia, ctx, d_counts, d_choices, np.floor(quant), W, H)
    d = (rgb.astype(np.int64) - decoded.astype(np.int64)) ** 2
    want = np.zeros(tx * ty, np.int64)
    for x in range(tx):                                       # t = tx * tiles_y + ty: x outer, y inner
        for y in range(ty):
            want[x * ty + y] = d[8 * y:8 * y + 8, 8 * x:8 * x + 8].sum()
    assert np.array_equal(tiles.astype(np.int64), want)
    assert int(d_sse.item()) == int(want.sum()) == _sse(rgb, decoded)
    # d_sse accumulates: a second call adds the same sum
    ctx.distortion_device(d_counts.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), W, H, d_sse.data_ptr(), quant=quant)
    torch.cuda.synchronize()
    assert int(d_sse.item()) == 2 * int(want.sum())


def test_full_size_frames(ia, oracle, photo):
    import torch
    ctx = _context(ia, 32)
    for rgb in (_synthetic(oracle, 4928, 3264, 12345), photo):
        H, W = rgb.shape[:2]
        d_rgb = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
        torch.cuda.synchronize()
        points = ctx.rate_distortion_device(d_rgb.data_ptr(), W, H, [8.0, 3.5, 1.0], keep_bytes=True)
        for p in points:
            _check_point(ia, ctx, rgb, p)
        host = ctx.rate_distortion(rgb, [8.0, 3.5, 1.0])
        assert [(p.size, p.sse, p.psnr) for p in host] == [(p.size, p.sse, p.psnr) for p in points]


def test_context_is_left_as_found(ia, oracle):
    ctx = _context(ia, 32)
    workgroups = ctx.L.mpc_context_tile_encode_workgroups
    workgroups.argtypes = [C.c_void_p]
    workgroups.restype = C.c_int
    before_q = ctx.quant.copy()
    rgb = _synthetic(oracle, 203, 117, 41)
    for wg in (0, 100):
        ctx.set_tile_encode_workgroups(wg)
        ctx.rate_distortion(rgb, LEVELS)
        assert workgroups(ctx.h) == wg
        assert np.array_equal(ctx.quant, before_q)
        assert not ctx.fast
    ctx.set_tile_encode_workgroups(0)
    fctx = _context(ia, 8, True)
    fctx.rate_distortion(rgb, [3.5])
    assert fctx.fast
    # an encode right after a sweep still gives the golden bytes
    with open(os.path.join(GOLDEN, "frames.json")) as f:
        frames = json.load(f)
    spec = next(s for s in frames.values() if s["kind"] == "synthetic" and s["width"] == 1003 and s["K"] == 32
                and s.get("flavour", "double") != "fast")
    from bench import synth_frame
    golden = synth_frame(spec["width"], spec["height"], spec["seed"])
    ctx.rate_distortion(golden, [8.0, 2.0])
    assert hashlib.sha256(ctx.encode_image(golden)).hexdigest() == spec["container_sha256"]
