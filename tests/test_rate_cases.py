"""A delta stream to a byte budget on the host: mpc_owed_tiles and mpc_budget_allocate_floor against the numpy models of
tests/rate_cases.py, the cases against the mistakes they are there to catch, the declared symbols, refusals, and the whole stream
replayed on the CPU with the oracle: records from the oracle's encoder, the profile from the oracle's decode of cut records,
containers from mpc_write_compressed, weights from mpc_container_index2, patches from mpc_patch_make.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import budget_cases as bc
import delta_cases as dc
import rate_cases as rc
from conftest import ROOT

ALLOCATE = rc.allocate_cases()
OWED = rc.owed_cases()
GATHER = rc.gather_cases()


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


# ---- the two host functions ----
@pytest.mark.parametrize("case", OWED, ids=[c[0] for c in OWED])
def test_owed_tiles_is_the_model(ia, case):
    name, sent, counts, K, changed = case
    cand, floor, must = ia.owed_tiles(sent, counts, K, changed)
    want = rc.owed_tiles(sent, counts, K, changed)
    assert cand.dtype == np.int32 and floor.dtype == np.uint8 and must.dtype == np.uint8
    for got, w in zip((cand, floor, must), want):
        assert got.shape == w.shape and (got == w).all(), name
    assert (np.diff(cand) > 0).all() and set(changed.tolist()) <= set(cand.tolist())
    if "nothing owed" in name:
        assert cand.size == 0
    if "sent 0" in name:
        assert cand.tolist() == np.flatnonzero(counts.any(axis=1)).tolist()


@pytest.mark.parametrize("case", ALLOCATE, ids=[c[0] for c in ALLOCATE])
def test_allocate_floor_is_the_model(ia, case):
    name, P, counts, floor, must, W, js = case
    K = P.shape[1] - 1
    for j in js:
        depth, cut, send, totals = ia.budget_allocate_floor(P, counts, floor, must, W, j)
        want_depth, want_cut, want_send, want_totals = rc.allocate_floor(P, counts, floor, must, W, j)
        assert (depth == want_depth).all() and (cut == want_cut).all() and (send == want_send).all(), (name, j)
        assert [int(v) for v in totals] == want_totals, (name, j)
        if must is None or must.all():                                             # mpc_budget_allocate bit for bit
            d0, c0, t0 = ia.budget_allocate(P, counts, W, j)
            assert (depth == d0).all() and (cut == c0).all() and [int(v) for v in totals[:3]] == [int(v) for v in t0], (name, j)
            assert send.all() and int(totals[3]) == P.shape[0]
        if must is not None and not must.any():                                    # nothing below a floor, and what stays is not sent
            low = np.minimum(floor, K)
            assert (depth >= low).all() and ((depth > low) == (send != 0)).all(), (name, j)
            if j == 255:
                assert (depth == low).all() and not send.any() and int(totals[1]) == 0 and int(totals[2]) == 0


def test_the_cases_cover_what_the_contract_names():
    names = [c[0] for c in ALLOCATE]
    for K in (1, 8, 32):
        for kind in ("every tile must", "no tile must", "mixed"):
            assert any(n.startswith(f"K{K} ") and n.endswith(kind) for n in names), (K, kind)
    assert any("counts above K" in n for n in names) and any("exact ties" in n for n in names)
    assert set(rc.JS) == {0, 1, 127, 254, 255}
    seen = set()
    for name, P, counts, floor, must, W, js in ALLOCATE:
        if floor is None:
            continue
        K = P.shape[1] - 1
        full = rc.full_depth(counts, K)
        seen |= {"zero"} if (floor == 0).any() else set()
        seen |= {"middle"} if ((floor > 0) & (floor < full)).any() else set()
        seen |= {"full"} if ((floor == full) & (full < K) & (full > 0)).any() else set()
        seen |= {"K"} if (floor == K).any() else set()
        seen |= {"above K"} if (floor > K).any() else set()
    assert seen == {"zero", "middle", "full", "K", "above K"}


@pytest.mark.parametrize("mistake", rc.WRONG_ALLOCATIONS)
def test_the_cases_tell_the_model_from_a_wrong_allocation(ia, mistake):
    caught = []
    for name, P, counts, floor, must, W, js in ALLOCATE:
        if P.shape[0] > 100:
            continue
        for j in js:
            want, got = rc.allocate_floor(P, counts, floor, must, W, j), rc.allocate_floor(P, counts, floor, must, W, j, mistake)
            if any((a != b).any() for a, b in zip(want[:3], got[:3])) or want[3] != got[3]:
                caught.append((name, j))
    assert caught, mistake
    # and where the mistake shows, the host function is not the mistaken one
    name, j = caught[0]
    _, P, counts, floor, must, W, _ = next(c for c in ALLOCATE if c[0] == name)
    got, wrong = ia.budget_allocate_floor(P, counts, floor, must, W, j), rc.allocate_floor(P, counts, floor, must, W, j, mistake)
    assert any((a != b).any() for a, b in zip(got[:3], wrong[:3])) or [int(v) for v in got[3]] != wrong[3], mistake


@pytest.mark.parametrize("mistake", rc.WRONG_OWED)
def test_the_cases_tell_the_model_from_a_wrong_owed_list(ia, mistake):
    caught = [(sent, counts, K, changed) for name, sent, counts, K, changed in OWED
              if not np.array_equal(rc.owed_tiles(sent, counts, K, changed)[0], rc.owed_tiles(sent, counts, K, changed, mistake)[0])]
    assert caught, mistake
    sent, counts, K, changed = caught[0]
    assert not np.array_equal(ia.owed_tiles(sent, counts, K, changed)[0], rc.owed_tiles(sent, counts, K, changed, mistake)[0]), mistake


@pytest.mark.parametrize("mistake", rc.WRONG_GATHERS)
def test_the_cases_tell_the_model_from_a_wrong_gather(mistake):
    caught = []
    for name, counts, words, K, tiles, idx, depth, n, rows in GATHER:
        want, got = rc.gather(counts, words, tiles, idx, depth, n, K, rows), rc.gather(counts, words, tiles, idx, depth, n, K, rows, mistake)
        if (want[0] != got[0]).any() or (want[1] != got[1]).any():
            caught.append(name)
    assert caught, mistake


def test_the_gather_model_inverts_the_scatter_model():
    rng = np.random.default_rng(3)
    K, T = 8, 66
    counts, words = dc.records(T, K, 4)
    tiles = np.sort(rng.choice(T, 20, replace=False))
    pcounts, pwords, bad = rc.gather(counts, words, tiles, None, None, 20, K)
    assert not bad and pcounts.shape == (20, 3)
    blank_counts, blank_words = np.zeros_like(counts), np.zeros_like(words)
    back_counts, back_words, bad = dc.scatter(pcounts, pwords, tiles, blank_counts, blank_words)
    assert not bad and (back_counts[tiles] == counts[tiles]).all() and (back_words[tiles] == words[tiles]).all()
    for name, c, w, K, tiles, idx, depth, n, rows in rc.bad_gather_cases():
        assert rc.gather(c, w, tiles, idx, depth, n, K, rows)[2], name


# ---- the C ABI ----
def test_the_declared_symbols_exist(ia):
    L = ia.load_library()
    text = open(os.path.join(ROOT, "include", "mpcodec.h")).read()
    assert text.index("budget: encode to a byte budget") < text.index("rate: a delta stream to a byte budget") < text.index('"-s" patch statistics')
    section = text.split("rate: a delta stream to a byte budget")[1].split('"-s" patch statistics')[0]
    names = set(re.findall(r"\b(mpc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", "/*" + section, flags=re.S)))
    want = {"mpc_owed_tiles", "mpc_budget_allocate_floor", "mpc_owed_tiles_device", "mpc_gather_records_device", "mpc_budget_allocate_floor_device",
            "mpc_delta_encode_patch_budget", "mpc_delta_sent"}
    assert names == want, names ^ want
    for name in want:
        assert hasattr(L, name), name
    for name in ("owed_tiles", "budget_allocate_floor", "RateInfo"):
        assert hasattr(ia, name)
    for name in ("owed_tiles_device", "gather_records_device", "budget_allocate_floor_device"):
        assert hasattr(ia.CompressionContext, name)
    for name in ("encode_patch_budget", "encode_patch_budget_device", "sent"):
        assert hasattr(ia.DeltaEncoder, name)


def test_refusals(ia):
    L, A = ia.load_library(), ia.api.MPC_ERR_ARGUMENT
    u8, u16, u32, i32 = ia.api._u8p, ia.api._u16p, ia.api._u32p, ia.api._i32p
    u64 = ia.api.C.POINTER(ia.api.C.c_uint64)
    n = ia.api.C.c_int(0)
    sent, counts, changed = np.zeros(4, np.uint8), np.ones(12, np.uint16), np.array([1, 3], np.int32)
    owed = lambda s, c, T, K, ch, nch, out: L.mpc_owed_tiles(s, c, T, K, ch, nch, None, None, None, out)
    S, Cn, Ch = sent.ctypes.data_as(u8), counts.ctypes.data_as(u16), changed.ctypes.data_as(i32)
    assert owed(S, Cn, 4, 8, Ch, 2, ia.api.C.byref(n)) == ia.api.MPC_OK and n.value == 4       # the outputs may be null
    assert owed(S, Cn, 4, 8, None, 0, ia.api.C.byref(n)) == ia.api.MPC_OK
    assert owed(S, Cn, 0, 8, None, 0, ia.api.C.byref(n)) == ia.api.MPC_OK and n.value == 0
    for args in ((None, Cn, 4, 8, Ch, 2), (S, None, 4, 8, Ch, 2), (S, Cn, 4, 8, None, 2), (S, Cn, -1, 8, None, 0), (S, Cn, 4, 0, Ch, 2), (S, Cn, 4, 33, Ch, 2),
                 (S, Cn, 4, 8, Ch, -1), (S, Cn, 1, 8, Ch, 2)):
        assert owed(*args, ia.api.C.byref(n)) == A, args
    assert owed(S, Cn, 4, 8, Ch, 2, None) == A
    for bad in ([3, 1], [1, 1], [1, 4], [-1, 2]):                                  # not ascending, not distinct, outside the frame
        b = np.array(bad, np.int32)
        assert owed(S, Cn, 4, 8, b.ctypes.data_as(i32), 2, ia.api.C.byref(n)) == A, bad
    P, c, W, t = np.zeros(9, np.uint32), np.zeros(3, np.uint16), np.full(24, 256, np.uint32), np.zeros(4, np.uint64)
    alloc = lambda p, tiles, K, j, tot: L.mpc_budget_allocate_floor(p, c.ctypes.data_as(u16), None, None, tiles, K, W.ctypes.data_as(u32), j, None, None,
                                                                    None, tot)
    assert alloc(P.ctypes.data_as(u32), 1, 8, 3, t.ctypes.data_as(u64)) == ia.api.MPC_OK
    assert alloc(P.ctypes.data_as(u32), 0, 8, 3, t.ctypes.data_as(u64)) == ia.api.MPC_OK
    for tiles, K, j in ((-1, 8, 0), (1, 0, 0), (1, 33, 0), (1, 8, -1), (1, 8, 256)):
        assert alloc(P.ctypes.data_as(u32), tiles, K, j, t.ctypes.data_as(u64)) == A
    assert alloc(None, 1, 8, 0, t.ctypes.data_as(u64)) == A and alloc(P.ctypes.data_as(u32), 1, 8, 0, None) == A
    # the session entry points check their pointers and the budget before they look at the session
    out, nb, info = ia.api._u8p(), ia.api.C.c_size_t(0), ia.api.MpcRateInfo()
    px = np.zeros((8, 8, 3), np.uint8)
    byref = ia.api.C.byref
    assert L.mpc_delta_encode_patch_budget(None, px.ctypes.data, 0, None, 0, 1000, byref(out), byref(nb), byref(info)) == A
    assert L.mpc_delta_sent(None, None, 0, byref(n)) == A
    # a host-only context: the device entry points say so, and no session can be made on it
    host_only = ia.create_compression_context(8, 8, 3.5, device=-1)
    for call in (lambda: host_only.owed_tiles_device(1, 1, 4, 1, 1, 1, 1, 1), lambda: host_only.gather_records_device(1, 1, 4, 1, 2, 0, 0, 2, 64, 1, 1),
                 lambda: host_only.budget_allocate_floor_device(1, 1, 0, 0, 4, np.full((3, 8), 256, np.uint32), 0, 1, 1, 1, 1),
                 lambda: host_only.delta_encoder(8, 8)):
        with pytest.raises(ia.MpcError) as e:
            call()
        assert e.value.status == ia.api.MPC_ERR_NO_DEVICE
    host_only.close()


# ---- the whole stream on the CPU ----
class OraclePieces:
    """rate_cases.Replay's pieces with the oracle's encoder and decoder and the library's host-only functions"""

    def __init__(self, ia, oracle, name):
        self.ia, self.oracle, self.name = ia, oracle, name
        self.K = dc.SHAPES[name][2]
        self.octx = oracle.OracleContext(self.K, 8, dc.QUALITY)
        q = dc.quant(name)
        self.quant = np.asarray(ia.quant_tables(self.K, dc.QUALITY) if q is None else q, np.float64).reshape(3, self.K)
        self._records, self._tiles, self._header = {}, {}, None

    def records(self, px):
        key = np.asarray(px).tobytes()
        if key not in self._records:
            counts, delta, coef, _e, _s = self.octx.encode_tiles(np.ascontiguousarray(px), quant=self.quant)
            words = delta.astype(np.uint32) | (coef.astype(np.uint32) << 16)
            words[np.arange(self.K)[None, None, :] >= counts[:, :, None]] = 0
            self._records[key] = (counts, words)
        return self._records[key]

    def container(self, counts, words, W, H):
        K = self.K
        counts = np.asarray(counts, np.uint16).reshape(-1, 3)
        words = np.asarray(words, np.uint32).reshape(-1, 3, K)
        codes = []
        for ch in range(3):
            for i in range(K):
                live = counts[:, ch] > i
                codes.append((words[live, ch, i] & 0xFFFF).astype(np.uint16))
                codes.append((words[live, ch, i] >> 16).astype(np.uint16))
        return self.ia.write_compressed(W, H, K, 8, self.quant, counts.reshape(-1), codes)

    def weights(self, container):
        return self.ia.budget_weights(self.ia.container_index2(container, 0, self.ia.api.MPC_INDEX_EXPANDED))

    def header_quant(self):
        """the u16 steps a container's header carries, which is what every decoder multiplies with"""
        if self._header is None:
            blob = self.container(np.zeros((1, 3), np.uint16), np.zeros((1, 3, self.K), np.uint32), 8, 8)
            self._header = np.asarray(self.ia.read_compressed(blob)["quant"], np.float64).reshape(3, self.K)
        return self._header

    def decode_tile(self, counts, words):
        """one tile's records (counts [3], words [3, K]) -> its 8 x 8 x 3 pixels: the oracle's FromCoeffsDynamic per channel, then
        RGBFromYUV with the decoder's rounding and clamp.  _the_tile_decoder_is_the_oracles_decode holds it to mpo_decode_image"""
        key = (np.asarray(counts).tobytes(), np.asarray(words).tobytes())
        if key not in self._tiles:
            q = self.header_quant()
            Y, U, V = (self.octx.from_coeffs(ch, int(counts[ch]), words[ch] & 0xFFFF, words[ch] >> 16, quant=q[ch]) for ch in range(3))
            rgb = np.stack([Y + 1.13983 * V, Y - 0.39466 * U - 0.58060 * V, Y + 2.03211 * U], axis=1)
            rgb = np.where(rgb >= 0, np.floor(rgb + 0.5), np.ceil(rgb - 0.5))
            self._tiles[key] = np.clip(rgb, 0, 255).astype(np.uint8).reshape(8, 8, 3)
        return self._tiles[key]

    def decode(self, counts, words, W, H):
        """whole-frame records -> the frame [H, W, 3]"""
        tx, ty = dc.grid(W, H)
        out = np.zeros((8 * ty, 8 * tx, 3), np.uint8)
        counts = np.minimum(np.asarray(counts, np.int64).reshape(-1, 3), self.K)
        for t in range(tx * ty):
            cx, cy = divmod(t, ty)
            out[8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] = self.decode_tile(counts[t], np.asarray(words[t], np.uint32))
        return out[:H, :W]

    def decode_container(self, blob):
        """a container -> the frame, through the library's host parser and decode()"""
        st = self.ia.read_compressed(blob)
        W, H, K = st["W"], st["H"], st["K"]
        counts = np.asarray(st["lengths"], np.int64).reshape(-1, 3)
        words = np.zeros((counts.shape[0], 3, K), np.uint32)
        for ch in range(3):
            for i in range(K):
                live = counts[:, ch] > i
                d, k = st["codes"][2 * K * ch + 2 * i], st["codes"][2 * K * ch + 2 * i + 1]
                words[live, ch, i] = np.asarray(d, np.uint32) | (np.asarray(k, np.uint32) << 16)
        return self.decode(counts, words, W, H)

    def profile(self, px, counts, words):
        px = np.asarray(px)
        counts = np.asarray(counts, np.uint16).reshape(-1, 3)
        P = np.zeros((counts.shape[0], self.K + 1), np.int64)
        for n in range(self.K + 1):
            P[:, n] = rc.tile_sums(px, self.decode(np.minimum(counts, n), words, px.shape[1], px.shape[0]))
        return P.astype(np.uint32)

    def patch(self, w, h, sequence, tiles, container, key):
        return self.ia.patch_make(w, h, sequence, None if tiles is None else [int(t) for t in tiles], container, key=key)


@functools.lru_cache(maxsize=None)
def tight_stream(ia, oracle, name):
    return rc.tight_stream(OraclePieces(ia, oracle, name), name, host=ia)          # the two host functions run beside the models


def _the_tile_decoder_is_the_oracles_decode(ia, oracle, name):
    """the replay's profile and receiver decode tile by tile with the oracle's FromCoeffsDynamic; mpo_decode_image builds its
    dictionary for every call, so it is asked twice a shape here and not nine times a call"""
    w, h, K = dc.SHAPES[name]
    p = OraclePieces(ia, oracle, name)
    px = dc.sequence(name)[0]
    counts, words = p.records(px)
    full = p.container(counts, words, w, h)
    assert full == p.octx.encode_image(np.ascontiguousarray(px), quant=p.quant)
    for n in (K, 3):
        blob = p.container(np.minimum(counts, n), words, w, h)
        assert (p.decode_container(blob) == oracle.decode_image(blob)).all(), n


@pytest.mark.parametrize("name", ["ragged", "full"])
def test_the_stream_replayed_on_the_cpu(ia, oracle, name):
    """The conditions the GPU test relies on, and the invariant on the host: a receiver that applies the replay's patches holds the
    decode of the frame's full records cut to `sent`.  Seed 3 of delta_cases.sequence; the budget is 3 times (ragged) and 1.2 times
    (full) the first non-key call's all_bytes, not half of it: at 0.5, 1 and 2 (ragged) and at 0.5 and 1 (full) this replay stalls
    with 66, 66, 62 and 4, 4 tiles owed after 32 calls of the tail (rate_cases.FRACTIONS says why); at these it needs 6 and 4."""
    import patch_cases as pc
    w, h, K = dc.SHAPES[name]
    _the_tile_decoder_is_the_oracles_decode(ia, oracle, name)
    frames, budget, results = tight_stream(ia, oracle, name)
    base = len(rc.base_sequence(name))
    tail = len(results) - base
    assert 1 <= tail <= 32 and results[-1]["owed"] == 0, (tail, results[-1]["owed"])
    pieces = OraclePieces(ia, oracle, name)
    kept = None
    cut_somewhere = refined = False
    for i, (px, r) in enumerate(zip(frames, results)):
        assert len(r["patch"]) <= budget and r["size255"] + 1 <= budget and r["probes"] <= 9, i
        info = ia.patch_info(r["patch"])
        assert info["sequence"] == i and (i > 0 or info["key"] == 1)
        if r["lambda_index"] >= 0:
            cut_somewhere = True
            assert r["lo_bytes"] > budget, i                                           # lo infeasible, hi feasible
        container = r["patch"][info["container_offset"]:]
        listed = ia.patch_tiles(r["patch"]).tolist()
        if info["key"]:
            kept = pieces.decode_container(container)
        elif listed:
            kept = pc.unpack(pieces.decode_container(container), listed, kept)
        want = pieces.decode(np.minimum(r["counts"], r["sent"][:, None]), r["words"], w, h)
        assert (kept == want).all(), (name, i)
        if i >= base:                                                                # the static tail
            assert (r["sent"] >= results[i - 1]["sent"]).all() and r["owed"] <= results[i - 1]["owed"] and r["changed"] == 0
            refined = refined or r["sent_tiles"] > 0
    assert cut_somewhere and refined and results[0]["key"] == 1
    # nothing owed: the receiver holds the decode of the frame's whole container, and the next patch is the empty patch
    whole = pieces.container(results[-1]["counts"], results[-1]["words"], w, h)
    assert (kept == oracle.decode_image(whole)).all()
    again = rc.Replay(pieces, w, h, K)
    for px in frames:
        again.call(px, budget)
    last = again.call(frames[-1], budget)
    assert len(last["patch"]) == 40 and last["candidates"] == 0 and last["owed"] == 0
    # a budget below size(255) invalidates the session: the next call is a key frame
    small = rc.Replay(pieces, w, h, K)
    assert small.call(frames[0], 41) is None and small.call(frames[0], 1 << 40)["key_frame"] == 1
