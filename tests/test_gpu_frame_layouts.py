"""The tile encoders on padded, offset and batched frame layouts (run with -m gpu): mpc_encode_tiles_device,
mpc_encode_batch_device and the host form mpc_encode_tiles read a frame by pointer plus strides, and every other test hands them
tight frames straight from an allocator.  Here every layout of tests/layout_cases.py (test_layout_cases.py proves on the CPU which
branch of the pixel fetch each one reaches) goes through every entry point it permits, in both flavours, and must give the oracle's
records on the TIGHT frames, bit for bit -- once with every non-pixel byte of the parent buffer zero and once with a random fill
that never equals a neighbouring pixel; the two results must also be identical, so a read of padding cannot hide.

Every parent buffer exceeds its view by at least one row stride and 64 bytes on both sides: a wrong address reads poison, never
outside the allocation.  No test here depends on a fault to notice anything."""
import ctypes as C

import numpy as np
import pytest

import layout_cases as lc
from parity_compare import compare

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in lc.CASES]
FLAVOURS = pytest.mark.parametrize("fast", [False, True], ids=["double", "float"])


class _Env:
    """contexts and oracles of both flavours for K = 8 and K = 32, created once; oracle results cached per (case, flavour)"""

    def __init__(self, torch, ia, oracle, octx32):
        self.torch, self.ia, self.oracle = torch, ia, oracle
        self.octx = {8: oracle.OracleContext(8, 8, 3.5), 32: octx32}
        self.ofast = {K: oracle.OracleFastContext(o) for K, o in self.octx.items()}
        self.ctx = {(K, fast): ia.create_compression_context(K, 8, 3.5, device=0).set_fast(fast) for K in (8, 32) for fast in (False, True)}
        self._frames, self._want = {}, {}

    def oracle_for(self, K, fast):
        return (self.ofast if fast else self.octx)[K]

    def frames(self, case):
        if case.name not in self._frames:
            f = lc.case_frames(case, self.oracle.synth_frame)
            f.flags.writeable = False
            self._frames[case.name] = f
        return self._frames[case.name]

    def want(self, case, fast):
        """the oracle's whole-frame outputs on the tight frames, frames stacked: counts, deltaId, intCoeff, energy, swept"""
        key = (case.name, fast)
        if key not in self._want:
            o = self.oracle_for(case.K, fast)
            per_frame = [o.encode_tiles(np.ascontiguousarray(f)) for f in self.frames(case)]
            self._want[key] = tuple(np.concatenate([p[i] for p in per_frame]) for i in range(5))
        return self._want[key]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def env(oracle, octx32):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    e = _Env(torch, ia, oracle, octx32)
    yield e
    e.close()


def _outputs(torch, tiles, K, fill=0):
    mk = lambda shape, dt: torch.full(shape, fill, dtype=dt, device="cuda")      # noqa: E731
    return mk((tiles, 3), torch.int16), mk((tiles, 3, K), torch.int32), mk((tiles, 3), torch.float64), mk((tiles, 3), torch.int32)


def _to_host(env, outs):
    d_counts, d_choices, d_energy, d_swept = outs
    return (d_counts.cpu().numpy().view(np.uint16), d_choices.cpu().numpy().view(np.uint32).view(env.ia.api.CHOICE_DTYPE),
            d_energy.cpu().numpy(), d_swept.cpu().numpy().view(np.uint32))


def _device_encode(env, ctx, d_ptr, L, a, b, batch, frames=None, frame_stride=None):
    """one launch on frames at device address d_ptr -> host copies of counts, choices, energy, swept"""
    torch = env.torch
    tiles_x, _ = lc.tiles_of(L)
    frames = L.frames if frames is None else frames
    outs = _outputs(torch, frames * tiles_x * (b - a), ctx.K)
    ptrs = [t.data_ptr() for t in outs]
    if batch:
        ctx.encode_batch_device(d_ptr, frames, L.frame_stride if frame_stride is None else frame_stride, L.W, L.H, L.row_stride, a, b, *ptrs)
    else:
        ctx.encode_tiles_device(d_ptr, L.W, L.H, L.row_stride, a, b, *ptrs)
    torch.cuda.synchronize()
    return _to_host(env, outs)


def _run_case(env, case, fast, stripes, host=True):
    """every entry point the layout permits, under both poisons: each result is the oracle's; the poisons' results are identical"""
    torch, L, K = env.torch, case.layout, case.K
    ctx = env.ctx[(K, fast)]
    tiles_x, tiles_y = lc.tiles_of(L)
    frames = env.frames(case)
    whole = env.want(case, fast)
    results = {}
    for poison in lc.POISONS:
        parent, start = lc.embed(frames, L, poison)
        d_parent = torch.from_numpy(parent).cuda()
        assert d_parent.data_ptr() % 8 == 0, "the case's alignment claims assume an 8-byte aligned parent"
        assert lc.flag_set(L) == case.claims["flag"]
        d_ptr = d_parent.data_ptr() + start
        for (a, b) in [(0, tiles_y)] + list(stripes):
            want = lc.stripe_of(whole, L.frames, tiles_x, tiles_y, a, b)
            runs = {}
            if L.frames == 1:
                runs["tiles_device"] = _device_encode(env, ctx, d_ptr, L, a, b, batch=False)
                if (a, b) == (0, tiles_y):
                    runs["batch_device, one frame"] = _device_encode(env, ctx, d_ptr, L, a, b, batch=True, frames=1, frame_stride=0)
                if host:
                    runs["host"] = ctx.encode_tiles(lc.host_view(parent, start, L), a, b)
            else:
                runs["batch_device"] = _device_encode(env, ctx, d_ptr, L, a, b, batch=True)
            for entry, got in runs.items():
                try:
                    compare(got, want, K)
                except AssertionError as e:
                    raise AssertionError(f"{case.name} [{entry}, rows {a}:{b}, poison {poison}, {'float' if fast else 'double'}]: {e}") from e
                results[(poison, entry, a, b)] = got
    for (poison, entry, a, b), got in results.items():
        if poison == lc.POISONS[0]:
            other = results[(lc.POISONS[1], entry, a, b)]
            for x, y in zip(got, other):
                assert x.tobytes() == y.tobytes(), f"{case.name} [{entry}, rows {a}:{b}]: the padding's content changed the result"


@FLAVOURS
@pytest.mark.parametrize("case", lc.CASES, ids=CASE_IDS)
def test_layout_records_equal_oracle(env, case, fast):
    _run_case(env, case, fast, case.stripes)


def test_host_form_takes_the_view_without_a_copy(env):
    """api.encode_tiles hands a [H, W, 3] view with contiguous pixels to mpc_encode_tiles as it is (strides[0] = row_stride); a view
    it cannot pass (every second column) is made contiguous: both give the oracle's records of the pixels the view shows"""
    case = lc.BY_NAME["crop-41x27-at-55-37"]
    L, ctx = case.layout, env.ctx[(8, False)]
    frames = env.frames(case)
    parent, start = lc.embed(frames, L, "random")
    view = lc.host_view(parent, start, L)
    assert not view.flags.c_contiguous and view.strides == (288, 3, 1)
    compare(ctx.encode_tiles(view), env.want(case, False), 8)
    sparse = view[:, ::2]
    assert sparse.strides[1] == 6
    compare(ctx.encode_tiles(sparse), env.octx[8].encode_tiles(np.ascontiguousarray(sparse)), 8)


@pytest.mark.parametrize("name", lc.STEPS_PATH_CASES)
def test_steps_path_layouts(env, monkeypatch, name):
    """MPC_PATH=steps: mp_init_kernel has its own copy of the addressing (double flavour only: that path refuses the float one)"""
    monkeypatch.setenv("MPC_PATH", "steps")
    case = lc.BY_NAME[name]
    _run_case(env, case, False, case.stripes)


# ---- the sequence entry points: one arbitrary device pointer per frame ----------------------------------------------------

FRAME_MISALIGNMENTS = (0, 1, 3, 4, 7)


def _frames_at_odd_offsets(env, W, H, seed):
    """five frames inside ONE device buffer at byte offsets 0, 1, 3, 4 and 7 mod 8, non-zero filler between them ->
    (frames, device buffer, offsets)"""
    n = 3 * W * H
    slot = (n + 64 + 7) // 8 * 8
    frames = [env.oracle.synth_frame(W, H, seed + f) for f in range(len(FRAME_MISALIGNMENTS))]
    host = np.random.default_rng(seed).integers(1, 256, 64 + slot * len(frames) + 64).astype(np.uint8)
    offsets = [64 + slot * f + m for f, m in enumerate(FRAME_MISALIGNMENTS)]
    for f, off in zip(frames, offsets):
        host[off:off + n] = f.reshape(-1)
    d = env.torch.from_numpy(host).cuda()
    assert d.data_ptr() % 8 == 0 and [o % 8 for o in offsets] == list(FRAME_MISALIGNMENTS)
    return frames, d, offsets


@FLAVOURS
@pytest.mark.parametrize("size", [(64, 48), (70, 50)])
def test_sequence_encode_with_unaligned_frame_pointers(env, size, fast):
    W, H = size
    frames, d, offsets = _frames_at_odd_offsets(env, W, H, 7000 + W)
    ctx, o = env.ctx[(8, fast)], env.oracle_for(8, fast)
    blobs = ctx.encode_images_device([d.data_ptr() + off for off in offsets], W, H)
    for f, (blob, frame) in enumerate(zip(blobs, frames)):
        assert bytes(blob) == bytes(o.encode_image(frame)), (f, offsets[f] % 8)


def test_rate_distortion_at_an_odd_offset_equals_the_aligned_copy(env):
    W, H = 70, 50
    frames, d, offsets = _frames_at_odd_offsets(env, W, H, 7100)
    ctx = env.ctx[(8, False)]
    levels = [8.0, 3.5]
    f = 2
    assert offsets[f] % 2 == 1
    odd = ctx.rate_distortion_device(d.data_ptr() + offsets[f], W, H, levels, keep_bytes=True)
    aligned = env.torch.from_numpy(frames[f]).cuda()
    assert aligned.data_ptr() % 8 == 0
    ref = ctx.rate_distortion_device(aligned.data_ptr(), W, H, levels, keep_bytes=True)
    assert [p.container for p in odd] == [p.container for p in ref]
    assert [(p.size, p.sse, p.psnr) for p in odd] == [(p.size, p.sse, p.psnr) for p in ref]
    assert all(p.container for p in odd)


# ---- offsets beyond 2^32 --------------------------------------------------------------------------------------------------

BIG = 2 ** 32


@pytest.fixture(scope="module")
def big_buffer(env):
    """one uninitialised device buffer of 2^32 + 2^20 bytes; nothing touches it except the frames the tests write"""
    torch = env.torch
    try:
        buf = torch.empty(BIG + 2 ** 20, dtype=torch.uint8, device="cuda")
    except Exception as e:                                    # not a skip: without the buffer the offsets are not tested
        pytest.fail(f"cannot allocate the {BIG + 2 ** 20} byte device buffer: {e}")
    assert buf.data_ptr() % 8 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


BIG_LAYOUTS = {
    "frame-stride-aligned": lc.Layout(0, 192, BIG + 8, 2, 64, 48),          # (a) frame 1 starts at 2^32 + 8: 8-byte fetch
    "frame-stride-odd": lc.Layout(0, 192, BIG + 3, 2, 64, 48),              # (b) ... at 2^32 + 3: byte fetch
    "row-stride": lc.Layout(0, 2 ** 29 + 8, 0, 1, 24, 9),                   # (c) the last row starts at 2^32 + 64
}


def _big_case(env, big_buffer, name, fast):
    torch, L, K = env.torch, BIG_LAYOUTS[name], 8
    frames = np.stack([env.oracle.synth_frame(L.W, L.H, 8800 + 10 * len(name) + f) for f in range(L.frames)])
    last = 0
    for f in range(L.frames):
        for y in range(L.H):
            at = f * L.frame_stride + y * L.row_stride
            big_buffer[at:at + 3 * L.W].copy_(torch.from_numpy(frames[f, y].reshape(-1)))
            last = max(last, at)
    assert last >= BIG and last + 3 * L.W <= big_buffer.numel()
    o = env.oracle_for(K, fast)
    per_frame = [o.encode_tiles(f) for f in frames]
    want = tuple(np.concatenate([p[i] for p in per_frame]) for i in range(5))
    _, tiles_y = lc.tiles_of(L)
    got = _device_encode(env, env.ctx[(K, fast)], big_buffer.data_ptr(), L, 0, tiles_y, batch=True)
    compare(got, want, K)


@FLAVOURS
@pytest.mark.parametrize("name", list(BIG_LAYOUTS))
def test_offsets_beyond_4GiB(env, big_buffer, name, fast):
    """the kernels' byte offsets are 64-bit: a frame stride and a row stride that put pixels beyond 2^32"""
    _big_case(env, big_buffer, name, fast)


def test_offsets_beyond_4GiB_steps_path(env, big_buffer, monkeypatch):
    monkeypatch.setenv("MPC_PATH", "steps")
    _big_case(env, big_buffer, "frame-stride-aligned", False)


# ---- arguments ------------------------------------------------------------------------------------------------------------

ARG_W, ARG_H, ARG_K = 64, 48, 8
ARG_TILES_Y = 6
GOOD = dict(frames=1, frame_stride=0, width=ARG_W, height=ARG_H, row_stride=3 * ARG_W, begin=0, end=ARG_TILES_Y, null=None)
BAD_ARGUMENTS = {
    "row_stride = 3W - 1": dict(row_stride=3 * ARG_W - 1),
    "width = 0": dict(width=0),
    "height = 0": dict(height=0),
    "height = -1": dict(height=-1),
    "frames = 0": dict(frames=0),
    "frames = 2, frame_stride = row_stride * H - 1": dict(frames=2, frame_stride=3 * ARG_W * ARG_H - 1),
    "tile_row_end = tiles_y + 1": dict(end=ARG_TILES_Y + 1),
    "tile_row_begin = tile_row_end": dict(begin=3, end=3),
    "null frame": dict(null="rgb"),
    "null counts": dict(null="counts"),
    "null records": dict(null="choices"),
}
PATTERN = 0xA5


@pytest.mark.parametrize("entry", ["tiles_device", "batch_device", "host"])
def test_bad_arguments_are_refused_and_leave_the_outputs_alone(env, entry):
    """MPC_ERR_ARGUMENT from each stride-taking entry point, the pattern in the output buffers unchanged, and the oracle's records
    from the same context on the next valid call.  (frames and frame_stride exist in the batch form only.)"""
    torch, api = env.torch, env.ia.api
    ctx, Lib = env.ctx[(ARG_K, False)], env.ia.api.load_library()
    rgb = env.oracle.synth_frame(ARG_W, ARG_H, 4711)
    two = np.concatenate([rgb, rgb])                              # frames = 2 has two real frames behind the pointer
    tiles = 2 * (ARG_W // 8) * ARG_TILES_Y
    sizes = (tiles * 6, tiles * 3 * ARG_K * 4, tiles * 24, tiles * 12)      # counts u16, records u32 [K], energy f64, swept u32; x 3 channels
    if entry == "host":
        outs = [np.full(n, PATTERN, np.uint8) for n in sizes]
        out_ptrs = [o.ctypes.data_as(t) for o, t in zip(outs, (api._u16p, C.c_void_p, api._dp, api._u32p))]
        frame_ptr = two.ctypes.data_as(api._u8p)
        snapshot = lambda: [o.tobytes() for o in outs]                                 # noqa: E731
    else:
        d_outs = [torch.full((n,), PATTERN, dtype=torch.uint8, device="cuda") for n in sizes]
        out_ptrs = [C.c_void_p(t.data_ptr()) for t in d_outs]
        d_two = torch.from_numpy(two).cuda()
        frame_ptr = C.c_void_p(d_two.data_ptr())

        def snapshot():
            torch.cuda.synchronize()
            return [t.cpu().numpy().tobytes() for t in d_outs]
    before = snapshot()
    assert all(set(b) == {PATTERN} for b in before)

    def call(**changes):
        a = dict(GOOD, **changes)
        ptrs = [None if a["null"] == n else p for n, p in zip(("counts", "choices", "energy", "swept"), out_ptrs)]
        frame = None if a["null"] == "rgb" else frame_ptr
        if entry == "host":
            return Lib.mpc_encode_tiles(ctx.h, frame, a["width"], a["height"], a["row_stride"], a["begin"], a["end"], None, *ptrs)
        if entry == "tiles_device":
            return Lib.mpc_encode_tiles_device(ctx.h, frame, a["width"], a["height"], a["row_stride"], a["begin"], a["end"], None, *ptrs, 0, None)
        return Lib.mpc_encode_batch_device(ctx.h, frame, a["frames"], a["frame_stride"], a["width"], a["height"], a["row_stride"], a["begin"],
                                           a["end"], None, *ptrs, 0, None)

    tried = 0
    for what, changes in BAD_ARGUMENTS.items():
        if entry != "batch_device" and ("frames" in changes or "frame_stride" in changes):
            continue
        assert call(**changes) == api.MPC_ERR_ARGUMENT, what
        assert snapshot() == before, what
        tried += 1
    assert tried == (len(BAD_ARGUMENTS) if entry == "batch_device" else len(BAD_ARGUMENTS) - 2)
    # the same context, the next valid call
    want = env.octx[ARG_K].encode_tiles(rgb)
    assert call() == api.MPC_OK
    after = snapshot()
    one = tiles // 2
    got = (np.frombuffer(after[0], np.uint16).reshape(tiles, 3)[:one], np.frombuffer(after[1], np.uint32).reshape(tiles, 3, ARG_K)[:one].view(api.CHOICE_DTYPE),
           np.frombuffer(after[2], np.float64).reshape(tiles, 3)[:one], np.frombuffer(after[3], np.uint32).reshape(tiles, 3)[:one])
    compare(got, want, ARG_K)
    for buf, n in zip(after, sizes):
        assert set(buf[n // 2:]) == {PATTERN}, "the valid one-frame call wrote beyond its tiles"
