"""A delta stream to a byte budget on the GPU (run with -m gpu): the three kernels against the host functions and the models of
tests/rate_cases.py, and the session's budget call: an unlimited budget gives mpc_delta_encode_patch's patches, a key call gives
mpc_encode_image_budget_device's container, and under a tight budget every patch is the replay's, byte for byte, the sent map is the
replay's, and a receiver that applies the patches holds the decode of the frame's full records cut to the sent map.  Refusals leave
the session as it was.  Every equality is exact.

The shapes are delta_cases.SHAPES (83x45: 66 tiles, ragged both ways, a packed frame with padding tiles; 16x16 at K = 32: full-length
records; 200x136: 425 tiles, seven packed columns; 5x3 and 8x8: one tile).  The tight budgets and the static tails come from
rate_cases.tight_stream, which says why they are what they are."""
import numpy as np
import pytest

import delta_cases as dc
import rate_cases as rc

pytestmark = pytest.mark.gpu

ALLOCATE = rc.allocate_cases()
OWED = rc.owed_cases()
GATHER = rc.gather_cases()


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def ctxs(ia):
    made = {K: ia.create_compression_context(K, 8, dc.QUALITY, device=0) for K in (1, 8, 32)}
    yield made
    for c in made.values():
        c.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(np.array(a.view(signed) if signed else a)).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _shifted(a, by, fill=0x5A):
    """the array in device memory `by` elements behind an aligned base -> (the window, the whole buffer)"""
    import torch
    whole = _dev(np.concatenate([np.full(by, fill, a.dtype), np.ascontiguousarray(a).reshape(-1)]))
    return whole[by:], whole


# ---- 1. the kernels ----
@pytest.mark.parametrize("K", (1, 8, 32))
def test_owed_flags_kernel_is_the_host_function(ia, ctxs, K):
    import torch
    ctx = ctxs[K]
    mine = [c for c in OWED if c[3] == K]
    assert len(mine) >= 15
    for k, (name, sent, counts, _, changed) in enumerate(mine):
        T = sent.shape[0]
        flags = np.zeros(T, np.uint8)
        flags[changed] = 1 + (np.arange(changed.size) % 3 == 0) * 4                    # any value but 0 means changed
        by = k % 2                                                                     # every other case on bases that are not aligned
        d_sent, _a = _shifted(sent, by)
        d_counts, _b = _shifted(counts.reshape(-1), by)
        d_flags, _c = _shifted(flags, by)
        d_floor = torch.full((T + by,), 0x77, dtype=torch.uint8, device="cuda")[by:]
        d_must = torch.full((T + by,), 0x77, dtype=torch.uint8, device="cuda")[by:]
        d_list = torch.full((T,), -7, dtype=torch.int32, device="cuda")
        d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        ctx.owed_tiles_device(d_sent.data_ptr(), d_counts.data_ptr(), T, d_flags.data_ptr(), d_floor.data_ptr(), d_must.data_ptr(), d_list.data_ptr(),
                              d_count.data_ptr())
        torch.cuda.synchronize()
        cand, floor, must = ia.owed_tiles(sent, counts, K, changed)
        model = rc.owed_tiles(sent, counts, K, changed)
        n = int(d_count.cpu()[0])
        assert n == cand.size == model[0].size, name
        assert (d_list.cpu().numpy()[:n] == cand).all() and (d_list.cpu().numpy()[n:] == -7).all(), name
        assert (_host(d_floor, np.uint8) == floor).all() and (_host(d_must, np.uint8) == must).all(), name
        got_flags = _host(d_flags, np.uint8)
        assert ((got_flags != 0) == np.isin(np.arange(T), cand)).all(), name
        assert (_host(d_sent, np.uint8) == sent).all() and (_host(d_counts, np.uint16) == counts.reshape(-1)).all()


def _gather_device(ctx, counts, words, K, tiles, idx, depth, n, rows, by=0, check=True):
    import torch
    T, m = counts.shape[0], len(tiles)
    R, Cc, _, _ = dc.pack_geometry(n, rows)
    P = R * Cc
    d_counts, _a = _shifted(counts.reshape(-1), by)
    d_words, _b = _shifted(words.reshape(-1), by)
    d_list = _dev(np.asarray(tiles, np.int32))
    d_idx = None if idx is None else _dev(np.asarray(idx, np.int32))
    d_depth = None if depth is None else _shifted(np.asarray(depth, np.uint8), by)[0]
    out_counts = torch.full((3 * P + by + 8,), 0x2A2A, dtype=torch.int16, device="cuda")
    out_words = torch.full((3 * P * K + by + 8,), 0x2A2A2A2A, dtype=torch.int32, device="cuda")
    ctx.gather_records_device(d_counts.data_ptr(), d_words.data_ptr(), T, d_list.data_ptr(), m, 0 if d_idx is None else d_idx.data_ptr(),
                              0 if d_depth is None else d_depth.data_ptr(), n, rows, out_counts[by:].data_ptr(), out_words[by:].data_ptr(), check=check)
    torch.cuda.synchronize()
    got_counts, got_words = _host(out_counts, np.uint16), _host(out_words, np.uint32)
    # nothing in front of the window, nothing behind the packed records
    assert (got_counts[:by] == 0x2A2A).all() and (got_counts[by + 3 * P:] == 0x2A2A).all()
    assert (got_words[:by] == 0x2A2A2A2A).all() and (got_words[by + 3 * P * K:] == 0x2A2A2A2A).all()
    assert (_host(d_counts, np.uint16) == counts.reshape(-1)).all() and (_host(d_words, np.uint32) == words.reshape(-1)).all()
    return got_counts[by:by + 3 * P].reshape(P, 3), got_words[by:by + 3 * P * K].reshape(P, 3, K)


@pytest.mark.parametrize("K", (1, 8, 32))
def test_gather_kernel_is_the_model(ia, ctxs, K):
    ctx = ctxs[K]
    mine = [c for c in GATHER if c[3] == K]
    assert len(mine) >= 20
    for k, (name, counts, words, _, tiles, idx, depth, n, rows) in enumerate(mine):
        for by in ((0, 1) if k % 3 == 0 else (0,)):                                     # 16-byte pieces, and the word path on a base 4 bytes off
            got_counts, got_words = _gather_device(ctx, counts, words, K, tiles, idx, depth, n, rows, by)
            want_counts, want_words, bad = rc.gather(counts, words, tiles, idx, depth, n, K, rows)
            assert not bad and (got_counts == want_counts).all() and (got_words == want_words).all(), (name, by)


def test_gather_is_the_scatter_turned_round(ia, ctxs):
    """records gathered uncut and scattered again land where they came from"""
    import torch
    ctx, K, T = ctxs[8], 8, 425
    counts, words = dc.records(T, K, 6)
    tiles = np.sort(np.random.default_rng(8).choice(T, 130, replace=False)).astype(np.int32)
    pcounts, pwords = _gather_device(ctx, counts, words, K, tiles, None, None, 130, dc.PACK_ROWS)
    d_counts = torch.zeros((T * 3,), dtype=torch.int16, device="cuda")
    d_words = torch.zeros((T * 3 * K,), dtype=torch.int32, device="cuda")
    d_pcounts, d_pwords, d_tiles = _dev(pcounts), _dev(pwords), _dev(tiles)
    ctx.scatter_records_device(d_pcounts.data_ptr(), d_pwords.data_ptr(), d_tiles.data_ptr(), 130, d_counts.data_ptr(), d_words.data_ptr(), T)
    torch.cuda.synchronize()
    back_counts, back_words = _host(d_counts, np.uint16).reshape(T, 3), _host(d_words, np.uint32).reshape(T, 3, K)
    assert (back_counts[tiles] == counts[tiles]).all() and (back_words[tiles] == words[tiles]).all()
    others = np.setdiff1d(np.arange(T), tiles)
    assert not back_counts[others].any() and not back_words[others].any()


def test_gather_entries_outside_their_range(ia, ctxs):
    ctx = ctxs[8]
    for name, counts, words, K, tiles, idx, depth, n, rows in rc.bad_gather_cases():
        want_counts, want_words, bad = rc.gather(counts, words, tiles, idx, depth, n, K, rows)
        assert bad
        with pytest.raises(ia.MpcError) as e:
            _gather_device(ctx, counts, words, K, tiles, idx, depth, n, rows)
        assert e.value.status == ia.api.MPC_ERR_BITSTREAM, name
        assert ctx.L.mpc_crop_records_check(ctx.h, None) == ia.api.MPC_OK              # read and cleared
        got_counts, got_words = _gather_device(ctx, counts, words, K, tiles, idx, depth, n, rows, check=False)
        assert ctx.L.mpc_crop_records_check(ctx.h, None) == ia.api.MPC_ERR_BITSTREAM
        assert (got_counts == want_counts).all() and (got_words == want_words).all(), name
    # refused with nothing enqueued
    counts, words = dc.records(4, 8, 1)
    for bad_args in (dict(n=0), dict(m=0), dict(T=0), dict(rows=0), dict(n=3)):         # n above the list's length without an index
        v = dict(dict(T=4, m=2, n=2, rows=64), **bad_args)
        with pytest.raises(ia.MpcError) as e:
            ctx.gather_records_device(1, 1, v["T"], 1, v["m"], 0, 0, v["n"], v["rows"], 1, 1)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, bad_args


@pytest.mark.parametrize("K", (1, 8, 32))
def test_floor_allocation_kernel_is_the_host_function(ia, ctxs, K):
    import torch
    ctx = ctxs[K]
    mine = [c for c in ALLOCATE if c[1].shape[1] == K + 1]
    assert len(mine) >= 8
    for name, P, counts, floor, must, W, js in mine:
        n = P.shape[0]
        d_profile, d_counts = _dev(P), _dev(counts)
        d_floor = None if floor is None else _dev(floor)
        d_must = None if must is None else _dev(must)
        for j in js:
            d_depth = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            d_send = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
            d_cut = torch.full((n, 3), -1, dtype=torch.int16, device="cuda")
            d_totals = torch.full((4,), -1, dtype=torch.int64, device="cuda")
            ctx.budget_allocate_floor_device(d_profile.data_ptr(), d_counts.data_ptr(), 0 if d_floor is None else d_floor.data_ptr(),
                                             0 if d_must is None else d_must.data_ptr(), n, W, j, d_depth.data_ptr(), d_cut.data_ptr(), d_send.data_ptr(),
                                             d_totals.data_ptr())
            torch.cuda.synchronize()
            depth, cut, send, totals = ia.budget_allocate_floor(P, counts, floor, must, W, j)
            assert (_host(d_depth, np.uint8) == depth).all() and (_host(d_send, np.uint8) == send).all(), (name, j)
            assert (_host(d_cut, np.uint16) == cut).all(), (name, j)
            assert [int(v) for v in _host(d_totals, np.uint64)] == [int(v) for v in totals], (name, j)
            if must is None:                                                           # mpc_budget_allocate_device, bit for bit
                b_depth = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
                b_cut = torch.full((n, 3), -1, dtype=torch.int16, device="cuda")
                b_totals = torch.full((3,), -1, dtype=torch.int64, device="cuda")
                ctx.budget_allocate_device(d_profile.data_ptr(), d_counts.data_ptr(), n, W, j, b_depth.data_ptr(), b_cut.data_ptr(), b_totals.data_ptr())
                torch.cuda.synchronize()
                assert (b_depth == d_depth).all() and (b_cut == d_cut).all() and (b_totals == d_totals[:3]).all(), (name, j)


# ---- 2. the session ----
class DevicePieces:
    """rate_cases.Replay's pieces from the context's public device entry points: the tile encoder, the depth profile, records -> container"""

    def __init__(self, ia, ctx, name):
        self.ia, self.ctx, self.K, self.q = ia, ctx, ctx.K, dc.quant(name)
        self._records = {}

    def records(self, px):
        key = (self.ctx.fast, np.asarray(px).tobytes())
        if key not in self._records:
            counts, choices, _e, _s = self.ctx.encode_tiles(np.ascontiguousarray(px), quant=self.q)
            self._records[key] = (np.array(counts, np.uint16), np.ascontiguousarray(choices).view(np.uint32).reshape(counts.shape[0], 3, self.K).copy())
        return self._records[key]

    def container(self, counts, words, W, H):
        import torch
        d_counts = _dev(np.concatenate([np.asarray(counts, np.uint16).reshape(-1), np.zeros(2, np.uint16)]))
        d_words = _dev(np.asarray(words, np.uint32).reshape(-1))
        torch.cuda.synchronize()
        return bytes(self.ctx.records_to_container_device(d_counts.data_ptr(), d_words.data_ptr(), W, H, quant=self.q))

    def weights(self, container):
        return self.ia.budget_weights(self.ia.container_index2(container, 0, self.ia.api.MPC_INDEX_EXPANDED))

    def profile(self, px, counts, words):
        import torch
        counts = np.asarray(counts, np.uint16).reshape(-1, 3)
        d_counts, d_words, d_px = _dev(counts), _dev(np.asarray(words, np.uint32).reshape(-1)), _dev(np.asarray(px))
        d_profile = torch.full((counts.shape[0], self.K + 1), -1, dtype=torch.int32, device="cuda")
        self.ctx.depth_profile_device(d_counts.data_ptr(), d_words.data_ptr(), d_px.data_ptr(), px.shape[1], px.shape[0], d_profile.data_ptr(), quant=self.q)
        torch.cuda.synchronize()
        return _host(d_profile, np.uint32)

    def patch(self, w, h, sequence, tiles, container, key):
        return self.ia.patch_make(w, h, sequence, None if tiles is None else [int(t) for t in tiles], container, key=key)

    def decode_cut(self, px, sent, header_quant):
        """mpc_decode_tiles_device of the frame's full records with every count cut to `sent`"""
        import ctypes as C
        import torch
        counts, words = self.records(px)
        d_counts, d_words = _dev(np.minimum(counts, np.asarray(sent, np.uint16)[:, None])), _dev(words.reshape(-1))
        out = torch.zeros((px.shape[0], px.shape[1], 3), dtype=torch.uint8, device="cuda")
        q = np.ascontiguousarray(header_quant, np.float64)
        assert self.ctx.L.mpc_decode_tiles_device(self.ctx.h, d_counts.data_ptr(), d_words.data_ptr(), q.ctypes.data_as(C.POINTER(C.c_double)), px.shape[1],
                                                  px.shape[0], out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _ctx(ctxs, name):
    return ctxs[dc.SHAPES[name][2]]


def _tiles(name):
    w, h, _ = dc.SHAPES[name]
    return dc.grid(w, h)[0] * dc.grid(w, h)[1]


@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_an_unlimited_budget_gives_the_unbudgeted_patches(ia, ctxs, name):
    """twin sessions over a whole sequence: budget 2^40 on one, mpc_delta_encode_patch on the other"""
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    T = _tiles(name)
    frames = dc.sequence(name) + [np.array(dc.frame(w, h, 77))]
    frames += [frames[-1], dc.change_tiles(frames[-1], [0, T - 1], 5)]
    a, b = ctx.delta_encoder(w, h), ctx.delta_encoder(w, h)
    with pytest.raises(ia.MpcError) as e:
        a.sent()
    assert e.value.status == ia.api.MPC_ERR_ARGUMENT                                  # a fresh session has no map
    for i, px in enumerate(frames):
        got, info = a.encode_patch_budget(px, 1 << 40, quant=dc.quant(name))
        want = b.encode_patch(px, quant=dc.quant(name))
        assert got == want, (name, i)
        assert (info.tiles, info.changed, info.key) == b.info == a.info and (a.changed() == b.changed()).all()
        assert info.lambda_index == -1 and info.probes == 0 and info.owed == 0 and info.candidates == info.changed == info.sent_tiles
        assert info.all_bytes == len(got) and (a.sent() == K).all() and a.sent().dtype == np.uint8 and a.sent().size == T
    a.close()
    b.close()


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", ["ragged", "full", "many"])
def test_a_key_call_is_the_single_frame_budget_encode(ia, ctxs, name, fast):
    import torch
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    px = np.array(dc.frame(w, h, 21))
    try:
        ctx.set_fast(fast)
        full = ctx.encode_image(px, quant=dc.quant(name))
        d_px = _dev(px)
        enc = ctx.delta_encoder(w, h)
        T = _tiles(name)
        smallest = 40 + len(DevicePieces(ia, ctx, name).container(np.zeros((T, 3), np.uint16), np.zeros((T, 3, K), np.uint32), w, h))
        assert smallest < len(full)
        for budget in (len(full) + 40, len(full) + 39, max(len(full) // 2 + 40, smallest + 100), max(len(full) // 4 + 40, smallest)):
            patch, info = enc.encode_patch_budget(px, budget, quant=dc.quant(name), key=True)
            want = ctx.encode_image_budget_device(d_px.data_ptr(), w, h, budget - 40, quant=dc.quant(name))
            pinfo = ia.patch_info(patch)
            assert pinfo["key"] == 1 and len(patch) <= budget and patch[pinfo["container_offset"]:] == want.container, (name, budget)
            assert (info.lambda_index, info.probes, info.sse) == (want.lambda_index, want.probes, want.sse), (name, budget)
            assert info.all_bytes == len(full) + 40 and (enc.sent() == want.depth).all() and info.key == 1 and info.sent_tiles == info.tiles
        enc.close()
    finally:
        ctx.set_fast(False)


_REPLAYS = {}


def _replay(ia, ctx, name):
    """rate_cases.tight_stream with this context's pieces, once per shape and flavour"""
    key = (name, ctx.fast)
    if key not in _REPLAYS:
        pieces = DevicePieces(ia, ctx, name)
        _REPLAYS[key] = (pieces,) + rc.tight_stream(pieces, name)
    return _REPLAYS[key]


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", list(dc.SHAPES))
def test_the_stream(ia, ctxs, name, fast):
    """delta_cases.sequence (single tiles changing, an unchanged frame among them) and a static tail under the tight budget of
    rate_cases.tight_stream: seed 3, 3 / 1.2 / 12 times the first non-key call's all_bytes for ragged / full / many, where the CPU
    replay reaches owed == 0 after 6 / 4 / 8 calls of the tail (half of it stalls: rate_cases.FRACTIONS); the sequences of one tile
    end in a flat frame that fits whole (rate_cases.base_sequence).  The device has to take exactly the replay's calls."""
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    T = _tiles(name)
    base = len(rc.base_sequence(name))
    try:
        ctx.set_fast(fast)
        pieces, frames, budget, results = _replay(ia, ctx, name)
        tail = len(results) - base
        # the same call count as the replay: asserted call by call below.  A frame of one tile ends flat and fits whole: no tail
        assert (0 if name in rc.ONE_TILE else 1) <= tail <= 32 and results[-1]["owed"] == 0
        enc, dec = ctx.delta_encoder(w, h), ctx.patch_decoder(w, h)
        header_quant = None
        cut = refined = False
        for i, (px, r) in enumerate(zip(frames, results)):
            d_px = _dev(px)                                                            # host pixels and device pixels in turn
            patch, info = (enc.encode_patch_budget(px, budget, quant=dc.quant(name)) if i % 2 == 0 else
                           enc.encode_patch_budget_device(d_px.data_ptr(), budget, quant=dc.quant(name)))
            assert len(patch) <= budget and patch == r["patch"], (name, fast, i, info)
            sent = enc.sent()
            assert (sent == r["sent"]).all(), (name, fast, i)
            for field in ("changed", "candidates", "sent_tiles", "owed", "lambda_index", "probes", "all_bytes", "key"):
                assert getattr(info, field) == r[field], (name, fast, i, field, info)
            if r["lambda_index"] >= 0:
                assert info.sse == r["sse"] and r["lo_bytes"] > budget
                cut = True
            dec.apply(patch)
            if header_quant is None:
                pinfo = ia.patch_info(patch)
                header_quant = ia.read_compressed(patch[pinfo["container_offset"]:])["quant"]
            assert (dec.frame() == pieces.decode_cut(px, sent, header_quant)).all(), (name, fast, i)      # THE INVARIANT
            if i >= base:
                assert (sent >= results[i - 1]["sent"]).all() and info.owed <= results[i - 1]["owed"] and info.changed == 0
                refined = refined or info.sent_tiles > 0
        assert cut and (refined or name in rc.ONE_TILE)
        # nothing is owed: the receiver holds what any decoder shows for the frame, and the next patch is the empty patch
        assert info.owed == 0
        whole = ctx.encode_image(np.ascontiguousarray(frames[-1]), quant=dc.quant(name))
        assert (dec.frame() == ctx.decode_images([whole])[0]).all()
        patch, info = enc.encode_patch_budget(frames[-1], budget, quant=dc.quant(name))
        assert len(patch) == 40 and (info.candidates, info.sent_tiles, info.owed, info.probes) == (0, 0, 0, 0)
        dec.apply(patch)
        assert (dec.frame() == ctx.decode_images([whole])[0]).all()
        enc.close()
        dec.close()
    finally:
        ctx.set_fast(False)


@pytest.mark.parametrize("name", ["ragged", "full"])
def test_the_stream_is_the_cpu_replays(ia, oracle, ctxs, name):
    """the oracle's encoder and decoder and the library's host functions alone give the patches the device gives"""
    import test_rate_cases as cpu
    ctx = _ctx(ctxs, name)
    _, frames, budget, results = _replay(ia, ctx, name)
    cpu_frames, cpu_budget, cpu_results = cpu.tight_stream(ia, oracle, name)
    assert budget == cpu_budget and len(results) == len(cpu_results)
    for i, (a, b) in enumerate(zip(results, cpu_results)):
        assert a["patch"] == b["patch"] and (a["sent"] == b["sent"]).all(), (name, i)


@pytest.mark.parametrize("name", ["ragged", "many"])
def test_a_probe_packs_more_tiles_than_the_frame_has(ia, ctxs, name):
    """Every tile a candidate, all but one of them sent: k = T - 1 lies in T's last partial packed column, so the probe's packed frame
    has 64 * ceil(k / 64) tiles -- 128 against 66, 448 against 425 -- and its records need room of their own size, not the frame's.
    A key frame cut to depth 0 leaves every tile owed; the next frame changes every tile but one, so probe(255) sends exactly T - 1."""
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    T = _tiles(name)
    pieces = DevicePieces(ia, ctx, name)
    first = np.array(dc.frame(w, h, 31))
    second = dc.change_tiles(first, [t for t in range(T) if t != T // 2], 4)
    replay = rc.Replay(pieces, w, h, K)
    zero = 40 + len(pieces.container(np.zeros((T, 3), np.uint16), np.zeros((T, 3, K), np.uint32), w, h))      # size(255) of a key frame
    want = [replay.call(first, zero)]
    assert want[0]["owed"] == T and not want[0]["sent"].any()
    loose = rc.Replay(pieces, w, h, K)
    loose.call(first, zero)
    budget = loose.call(second, 1 << 40)["all_bytes"] // 2
    want.append(replay.call(second, budget))
    assert want[1] is not None and want[1]["candidates"] == T and want[1]["key_frame"] == 0 and want[1]["changed"] == T - 1
    assert T - 1 in replay.probed_k and dc.pack_geometry(T - 1)[0] * dc.pack_geometry(T - 1)[1] > T
    enc, dec = ctx.delta_encoder(w, h), ctx.patch_decoder(w, h)
    for px, room, r in ((first, zero, want[0]), (second, budget, want[1])):
        patch, info = enc.encode_patch_budget(px, room, quant=dc.quant(name))
        assert patch == r["patch"] and (enc.sent() == r["sent"]).all() and (info.owed, info.probes, info.lambda_index) == (r["owed"], r["probes"], r["lambda_index"])
        dec.apply(patch)
    header_quant = ia.read_compressed(pieces.container(np.zeros((T, 3), np.uint16), np.zeros((T, 3, K), np.uint32), w, h))["quant"]
    assert (dec.frame() == pieces.decode_cut(second, enc.sent(), header_quant)).all()
    enc.close()
    dec.close()


def _session_state(enc):
    return enc.sent().copy(), enc.changed().copy(), enc.info


def test_refusals_are_atomic(ia, ctxs):
    name = "ragged"
    ctx = _ctx(ctxs, name)
    w, h, K = dc.SHAPES[name]
    T = _tiles(name)
    A = ia.api.MPC_ERR_ARGUMENT
    pieces, frames, budget, results = _replay(ia, ctx, name)
    enc, dec = ctx.delta_encoder(w, h), ctx.patch_decoder(w, h)
    for i in range(3):
        patch, info = enc.encode_patch_budget(frames[i], budget)
        assert patch == results[i]["patch"]
        dec.apply(patch)
    # refused calls: the sent map, the list, the store and the sequence stay as they were
    before = _session_state(enc)
    r = pieces.records(frames[2])
    d_busy_counts, d_busy_words = _dev(r[0]), _dev(r[1].reshape(-1))
    ctx.container_job_begin(3, d_busy_counts.data_ptr(), d_busy_words.data_ptr(), w, h)
    ctx.kernel_timing(True)
    ctx.read_kernel_timing()
    strided = np.zeros((h, 3 * w - 3), np.uint8)
    for call, text in ((lambda: enc.encode_patch_budget(frames[3], 39), "39"), (lambda: enc.encode_patch_budget(frames[3], budget), "slot 3 is busy"),
                       (lambda: enc._encode_patch_budget(strided.ctypes.data, 3 * w - 1, budget, None, 0), "row_stride"),
                       (lambda: enc._encode_patch_budget(frames[3].ctypes.data, 0, budget, None, 64), "flags")):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == A and text in str(e.value), str(e.value)
    assert ctx.read_kernel_timing()[1] == 0                                          # no pursuit was launched
    ctx.kernel_timing(False)
    ctx.container_job_cancel(3)
    after = _session_state(enc)
    assert (after[0] == before[0]).all() and (after[1] == before[1]).all() and after[2] == before[2]
    patch, info = enc.encode_patch_budget(frames[3], budget)
    assert patch == results[3]["patch"] and ia.patch_info(patch)["sequence"] == 3     # still a delta, the next in sequence
    dec.apply(patch)
    # a budget below size(255): refused with both figures, the session invalidated -- the next call is a key frame
    smallest = results[4]["size255"]
    with pytest.raises(ia.MpcError) as e:
        enc.encode_patch_budget(frames[4], smallest - 1)
    assert e.value.status == A and str(smallest - 1) in str(e.value) and str(smallest) in str(e.value), str(e.value)
    with pytest.raises(ia.MpcError):
        enc.sent()
    patch, info = enc.encode_patch_budget(frames[4], 1 << 40)
    assert info.key == 1 and ia.patch_info(patch)["key"] == 1 and ia.patch_info(patch)["sequence"] == 4 and (enc.sent() == K).all()
    dec.apply(patch)
    whole = lambda px: ctx.decode_images([ctx.encode_image(np.ascontiguousarray(px))])[0]
    assert (dec.frame() == whole(frames[4])).all()
    # an unbudgeted call on a budgeted session: the map is gone, the next budget call is a key frame, and no receiver keeps a stale tile
    px = dc.change_tiles(frames[4], [1, T - 2], 9)
    dec.apply(enc.encode_patch(px))
    with pytest.raises(ia.MpcError):
        enc.sent()
    px2 = dc.change_tiles(px, [5], 10)
    patch, info = enc.encode_patch_budget(px2, budget)
    assert info.key == 1 and info.changed == T and ia.patch_info(patch)["key"] == 1 and len(patch) <= budget
    dec.apply(patch)
    header_quant = ia.read_compressed(patch[ia.patch_info(patch)["container_offset"]:])["quant"]
    assert (dec.frame() == pieces.decode_cut(px2, enc.sent(), header_quant)).all()
    enc.close()
    dec.close()
