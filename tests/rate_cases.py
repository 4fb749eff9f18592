"""A delta stream to a byte budget as numpy models (include/mpcodec.h, "rate"), the cases the host functions and the kernels are held
to, the mistakes those cases must tell apart, and the session's search as a function of public pieces.  Imported by
test_rate_cases.py (CPU) and test_gpu_rate.py; nothing here needs the library: whatever does (records, profile, container, weights,
patch) reaches the replay as a `pieces` object.

  owed_tiles      sent[T], counts[T, 3], the changed list -> the candidates (changed + owed, ascending), per tile floor and must
  gather          whole-frame records, a list, optionally an index into it and a depth per list entry -> the packed frame's records
  allocate_floor  budget_cases.allocate with a floor and a must byte per candidate
  Replay          mpc_delta_encode_patch_budget, call by call"""
import numpy as np

import budget_cases as bc
import delta_cases as dc

JS = (0, 1, 127, 254, 255)
FILL16, FILL32 = 0xA5A5, 0xA5A5A5A5            # what an output buffer holds before a gather: a missing zero shows


# ---- the models ----
def full_depth(counts, K, mistake=None):
    counts = np.minimum(np.asarray(counts, np.int64).reshape(-1, 3), K)
    return counts[:, 0] if mistake == "owed decided on one channel's count only" else counts.max(axis=1)


def owed_tiles(sent, counts, K, changed, mistake=None):
    """-> (candidates int32 ascending, floor uint8 [T], must uint8 [T])"""
    sent = np.asarray(sent, np.uint8)
    T = sent.shape[0]
    must = np.zeros(T, np.uint8)
    must[np.asarray(changed, np.int64)] = 1
    owed = sent.astype(np.int64) < full_depth(counts, K, mistake)
    cand = np.flatnonzero((must != 0) | owed).astype(np.int32)
    if mistake == "descending list":
        cand = cand[::-1].copy()
    return cand, np.where(must != 0, 0, sent).astype(np.uint8), must


def gather(counts, words, tiles, idx, depth, n, K, rows=dc.PACK_ROWS, mistake=None):
    """counts [T, 3], words [T, 3, K], tiles: the list; idx: None or n entries into it; depth: None or a depth per list entry ->
    (packed counts uint16 [P, 3], packed words uint32 [P, 3, K], an entry was outside its range), P = R * C of pack_geometry(n, rows)"""
    counts, words = np.asarray(counts, np.uint16).reshape(-1, 3), np.asarray(words, np.uint32).reshape(-1, 3, K)
    T, m = counts.shape[0], len(tiles)
    R, Cc, _, _ = dc.pack_geometry(n, rows)
    out_counts, out_words = np.full((R * Cc, 3), FILL16, np.uint16), np.full((R * Cc, 3, K), FILL32, np.uint32)
    bad = False
    for j in range(R * Cc):
        if j >= n:
            if mistake != "padding tiles not zeroed":
                out_counts[j], out_words[j] = 0, 0
            continue
        out_counts[j], out_words[j] = 0, 0
        c = j if idx is None else int(idx[j])
        if not 0 <= c < m or not 0 <= int(tiles[c]) < T:
            bad = True
            continue
        t = int(tiles[c])
        cut = K if depth is None else int(depth[c])
        for ch in range(3):
            keep = min(int(counts[t, ch]), K, cut)
            out_counts[j, ch] = keep
            upto = min(int(counts[t, ch]), K) if mistake == "entries above the cut not zeroed" else keep
            out_words[j, ch, :upto] = words[t, ch, :upto]
    return out_counts, out_words, bad


def allocate_floor(profile, counts, floor, must, weights, j, mistake=None):
    """-> (depth uint8 [n], cut counts uint16 [n, 3], send uint8 [n], totals [distortion, rate, records sent, tiles sent] as Python ints)"""
    profile = np.asarray(profile, np.uint32)
    n, K = profile.shape[0], profile.shape[1] - 1
    counts = np.minimum(np.asarray(counts, np.int64).reshape(n, 3), K)
    floor = np.zeros(n, np.int64) if floor is None else np.minimum(np.asarray(floor, np.int64), K)
    must = np.ones(n, np.int64) if must is None else np.asarray(must, np.int64)
    R = bc.rates(counts, weights, K)
    L = bc.lambda_of(j)
    depth, send = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    totals = [0, 0, 0, 0]
    for i in range(n):
        low = 0 if mistake == "floor ignored" else int(floor[i])
        free = not must[i]
        allowed = range(0, K + 1) if must[i] or mistake == "depths below the floor allowed" else range(low, K + 1)
        rate = {d: 0 if free and d == low and mistake != "staying charged at R[floor]" else R[i, d] for d in allowed}
        J = {d: int(profile[i, d]) * 65536 + L * rate[d] for d in allowed}
        best = min(J.values())
        at = [d for d in allowed if J[d] == best]
        depth[i] = at[-1] if mistake == "ties to the larger n" else at[0]
        send[i] = 1 if must[i] or depth[i] > low or mistake == "send for a tile that stays" else 0
        totals[0] += int(profile[i, depth[i]])
        totals[1] += rate[int(depth[i])]
        if send[i]:
            totals[2] += int(np.minimum(counts[i], int(depth[i])).sum())
            totals[3] += 1
    cut = np.minimum(counts, depth[:, None].astype(np.int64)).astype(np.uint16)
    return depth, cut, send, totals


WRONG_ALLOCATIONS = ("floor ignored", "staying charged at R[floor]", "depths below the floor allowed", "ties to the larger n",
                     "send for a tile that stays")
WRONG_GATHERS = ("entries above the cut not zeroed", "padding tiles not zeroed")
WRONG_OWED = ("owed decided on one channel's count only", "descending list")


# ---- the cases ----
def allocate_cases():
    """[(name, profile, counts, floor or None, must or None, weights, js)]: budget_cases' profiles (K in 1, 8, 32; ties; counts above K)
    with every tile must, no tile must, and a mix; floors 0, in the middle, equal to the tile's full depth, equal to K, above K"""
    rng = np.random.default_rng(20241020)
    out = []
    for name, P, counts, W, _ in bc.cases():
        T, K = P.shape[0], P.shape[1] - 1
        if T > 100:
            continue
        full = full_depth(counts, K)
        kinds = rng.integers(0, 5, T)
        floor = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3], [0, full // 2, full, K], rng.integers(0, K + 1, T)).astype(np.uint8)
        out.append((f"{name}: every tile must", P, counts, None, None, W, JS))
        out.append((f"{name}: every tile must, floors given", P, counts, floor, np.ones(T, np.uint8), W, JS))
        out.append((f"{name}: no tile must", P, counts, floor, np.zeros(T, np.uint8), W, JS))
        out.append((f"{name}: mixed", P, counts, floor, (rng.random(T) < 0.4).astype(np.uint8), W, JS))
    K, T = 8, 9
    counts = np.full((T, 3), K, np.uint16)
    P = np.maximum(3_000_000 - 300_000 * np.arange(K + 1, dtype=np.int64), 0)[None, :].repeat(T, 0).astype(np.uint32)
    out.append(("K8 a floor above K", P, counts, np.array([0, 3, 8, 9, 200, 255, 4, 8, 1], np.uint8), np.array([0, 0, 0, 0, 0, 0, 1, 1, 0], np.uint8),
                np.full((3, K), 1000, np.uint32), JS))
    K, T = 8, 4097                                       # more candidates than one launch's workgroups take in one round
    counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
    P = np.sort(rng.integers(0, bc.P_MAX, (T, K + 1)), axis=1)[:, ::-1].astype(np.uint32)
    out.append(("K8 T4097 mixed", P, counts, rng.integers(0, K + 1, T).astype(np.uint8), (rng.random(T) < 0.3).astype(np.uint8),
                np.full((3, K), 2000, np.uint32), (0, 127, 255)))
    return out


def owed_cases():
    """[(name, sent, counts, K, changed)]"""
    rng = np.random.default_rng(77)
    out = []
    for K in (1, 8, 32):
        for T in (1, 66, 1024, 1025, 2500):
            counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
            counts[rng.random(T) < 0.2] = 0
            if T > 5:
                counts[5, 1], counts[3, 2] = K + 1, 65535                    # used as K
            sent = np.where(rng.random(T) < 0.5, full_depth(counts, K), rng.integers(0, K + 1, T)).astype(np.uint8)
            for label, changed in (("none changed", []), ("some changed", np.flatnonzero(rng.random(T) < 0.3)), ("all changed", np.arange(T))):
                out.append((f"K{K} T{T} {label}", sent, counts, K, np.asarray(changed, np.int32)))
        T = 70                                                               # nothing owed: sent equal to full, and sent = K
        counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
        out.append((f"K{K} nothing owed", full_depth(counts, K).astype(np.uint8), counts, K, np.zeros(0, np.int32)))
        out.append((f"K{K} sent K", np.full(T, K, np.uint8), counts, K, np.array([0, T - 1], np.int32)))
        out.append((f"K{K} sent 0", np.zeros(T, np.uint8), counts, K, np.zeros(0, np.int32)))
    return out


def gather_cases():
    """[(name, counts, words, K, tiles, idx or None, depth or None, n, rows)]: hand-made records with garbage above every count -- the
    store's are zero there, the gather must not rely on it"""
    rng = np.random.default_rng(99)
    out = []
    for K in (1, 6, 8, 32):
        for T in (1, 66, 425):
            counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
            words = rng.integers(1, 2**32, (T, 3, K), dtype=np.uint64).astype(np.uint32)
            if T > 5:
                counts[2, 0] = K + 3                                             # used as K
            for m in sorted({1, min(T, 63), min(T, 64), min(T, 65), T}):
                tiles = np.sort(rng.choice(T, m, replace=False)).astype(np.int32)
                depth = rng.integers(0, K + 1, m).astype(np.uint8)
                out.append((f"K{K} T{T} m{m} uncut", counts, words, K, tiles, None, None, m, dc.PACK_ROWS))
                out.append((f"K{K} T{T} m{m} cut", counts, words, K, tiles, None, depth, m, dc.PACK_ROWS))
                n = max(1, m // 2)
                idx = np.sort(rng.choice(m, n, replace=False)).astype(np.int32)
                out.append((f"K{K} T{T} m{m} n{n} cut, indexed", counts, words, K, tiles, idx, depth, n, 3 if m < 10 else dc.PACK_ROWS))
    return out


def bad_gather_cases():
    """entries outside their ranges: that packed tile is all zero, the others are as they would be"""
    rng = np.random.default_rng(5)
    K, T = 8, 66
    counts = rng.integers(1, K + 1, (T, 3)).astype(np.uint16)
    words = rng.integers(1, 2**32, (T, 3, K), dtype=np.uint64).astype(np.uint32)
    depth = rng.integers(0, K + 1, 6).astype(np.uint8)
    return [("list entries outside the frame", counts, words, K, np.array([0, T, -1, 5, 2**31 - 1, T - 1], np.int32), None, depth, 6, 4),
            ("index entries outside the list", counts, words, K, np.array([0, 7, 9, 5, 11, T - 1], np.int32), np.array([0, 6, -1, 5], np.int32), depth, 4, 3)]


# ---- the session's search, call by call ----
def tile_sums(a, b):
    """per tile t = tx * tiles_y + ty the sum of squared differences of two [H, W, 3] frames"""
    H, W = a.shape[:2]
    d = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum(axis=2)
    full = np.zeros((-(-H // 8) * 8, -(-W // 8) * 8), np.int64)
    full[:H, :W] = d
    return full.reshape(full.shape[0] // 8, 8, full.shape[1] // 8, 8).sum(axis=(1, 3)).T.reshape(-1)


class Replay:
    """mpc_delta_encode_patch_budget with public pieces alone.  pieces:
         records(px) -> (counts uint16 [T, 3], words uint32 [T, 3, K]) of a whole frame
         profile(px, counts, words) -> [tiles, K + 1]: the frame's records against the frame (a whole one or a packed one)
         container(counts, words, W, H) -> bytes;  weights(container) -> uint32 [3, K];  patch(w, h, sequence, tiles, container, key) -> bytes
    host: None, or the library (imageexperiments_amd): then mpc_owed_tiles and mpc_budget_allocate_floor run beside the models on
    everything the stream feeds them and have to agree.
    One instance is one sender session; `unbudgeted()` is what a call of another kind does to it."""

    def __init__(self, pieces, w, h, K, host=None):
        self.p, self.w, self.h, self.K, self.host = pieces, w, h, K, host
        self.T = dc.grid(w, h)[0] * dc.grid(w, h)[1]
        self.sent, self.kept, self.calls = None, None, 0
        self.probed_k = []                                  # tiles sent by every probe so far

    def unbudgeted(self, px):
        self.sent, self.kept = None, np.array(px)
        self.calls += 1

    def call(self, px, budget, key=False):
        """-> dict(patch, key, changed, candidates, sent_tiles, owed, lambda_index, probes, all_bytes, sse, size255, sent), or None for
        a budget below size(255) (the session then wants a key frame)"""
        K, T, p = self.K, self.T, self.p
        key = key or self.sent is None or self.kept is None
        changed = np.arange(T, dtype=np.int32) if key else dc.changed_tiles(self.kept, px)
        self.kept = np.array(px)
        counts, words = p.records(px)
        if key:
            cand, floor_t, must_t = np.arange(T, dtype=np.int32), np.zeros(T, np.uint8), np.ones(T, np.uint8)
        else:
            cand, floor_t, must_t = owed_tiles(self.sent, counts, K, changed)
            if self.host is not None:
                got = self.host.owed_tiles(self.sent, counts, K, changed)
                assert all(np.array_equal(a, b) for a, b in zip(got, (cand, floor_t, must_t))), "mpc_owed_tiles is not the model"
        m = len(cand)
        out = dict(key=int(key), key_frame=int(key), changed=len(changed), candidates=m, lambda_index=-1, probes=0, sse=0, size255=40)
        empty = p.patch(self.w, self.h, self.calls, [], b"", False)
        sent = np.zeros(T, np.uint8) if self.sent is None else self.sent.copy()
        if m == 0:
            out.update(patch=empty, all_bytes=len(empty), sent_tiles=0)
        else:
            whole = m == T
            if whole:
                cpx, ccounts, cwords, W, H = px, counts, words, self.w, self.h
            else:
                ccounts, cwords, bad = gather(counts, words, cand, None, None, m, K)
                assert not bad
                cpx = dc.pack(px, [int(t) for t in cand])
                R, Cc, _, _ = dc.pack_geometry(m)
                W, H = 8 * Cc, 8 * R
            floor, must = floor_t[cand], must_t[cand]
            F = p.container(ccounts, cwords, W, H)
            everything = p.patch(self.w, self.h, self.calls, None if whole else cand, F, whole)
            out["all_bytes"] = len(everything)
            if len(everything) <= budget:
                sent[cand] = K
                P = None
                out.update(patch=everything, sent_tiles=m, key=int(key or whole))
            else:
                weights = p.weights(F)
                P = np.asarray(p.profile(cpx, ccounts, cwords))[:m]
                made = {}

                def size(j):
                    if j not in made:
                        depth, cut, send, totals = allocate_floor(P, ccounts[:m], floor, must, weights, j)
                        if self.host is not None:
                            got = self.host.budget_allocate_floor(P, ccounts[:m], floor, must, weights, j)
                            assert all(np.array_equal(a, b) for a, b in zip(got[:3], (depth, cut, send))), "mpc_budget_allocate_floor is not the model"
                            assert [int(v) for v in got[3]] == totals
                        idx = np.flatnonzero(send).astype(np.int32)
                        k = len(idx)
                        if k == 0:
                            blob = empty
                        elif k == T:
                            blob = p.patch(self.w, self.h, self.calls, None, p.container(cut, words, self.w, self.h), True)
                        else:
                            pcounts, pwords, bad = gather(counts, words, cand, idx, depth, k, K)
                            assert not bad
                            R, Cc, _, _ = dc.pack_geometry(k)
                            blob = p.patch(self.w, self.h, self.calls, cand[idx], p.container(pcounts, pwords, 8 * Cc, 8 * R), False)
                        made[j] = (blob, depth, idx, totals)
                        self.probed_k.append(k)
                    return made[j]

                out["size255"] = len(size(255)[0])
                if out["size255"] > budget:
                    self.refused_size255 = out["size255"]
                    self.sent = None
                    self.kept = None
                    return None
                lo, hi = -1, 255
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if len(size(mid)[0]) <= budget:
                        hi = mid
                    else:
                        lo = mid
                blob, depth, idx, totals = size(hi)
                sent[cand[idx]] = depth[idx]
                out.update(patch=blob, sent_tiles=len(idx), lambda_index=hi, probes=len(made), sse=totals[0], key=int(key or len(idx) == T))
                out["lo_bytes"] = len(size(lo)[0]) if lo >= 0 else len(everything)
        self.sent = sent
        self.calls += 1
        out["owed"] = int((sent.astype(np.int64) < full_depth(counts, K)).sum())
        out["sent"] = sent.copy()
        out["counts"], out["words"] = counts, words
        return out


# The tight budget of the stream tests.  The rule is: a fraction of the first non-key call's all_bytes in a stream that is never cut,
# rounded up, and at least size(255) + 1 of every call; the static tail is as long as the replay needs to reach owed == 0.  Half of
# that all_bytes does not get there on these sequences: every non-key frame of delta_cases.sequence changes a single tile, half of a
# one-tile patch is a few hundred bytes, and the search stalls -- at one multiplier no owed tile is worth its bytes, at the next one
# down too many are at once, so hi sends nothing, call after call.  (Found with the CPU replay, seed 3: ragged 0.5, 1 and 2 stall
# with 66, 66 and 62 tiles owed; full 0.5 and 1 with 4; many 0.5 to 8 with 425 to 404.)  The fractions below are the smallest tried
# at which the CPU replay reaches owed == 0 within 32 calls of the tail: ragged 3 -> 6 calls, full 1.2 -> 4, many 12 -> 8.
# A frame of one tile can never be refined under a budget below its all_bytes: a refined tile is sent from step 0, so its full records
# must fit one patch.  The sequences of `one` and `tiny` therefore end in a flat frame, whose records are few: the busy frames in
# front of it are cut (0.9 of their patch), the flat one fits whole, and the stream ends with nothing owed like the others.
FRACTIONS = {"ragged": 3, "full": 1.2, "many": 12, "one": 0.9, "tiny": 0.9}
ONE_TILE = ("one", "tiny")
SEED = 3


def base_sequence(name):
    """delta_cases.sequence(name), and behind it for the frames of one tile a flat frame"""
    w, h, _ = dc.SHAPES[name]
    base = dc.sequence(name, seed=SEED)
    return base + [np.full((h, w, 3), 128, np.uint8)] if name in ONE_TILE else base


def tight_stream(pieces, name, host=None):
    """the replay of base_sequence(name) plus a static tail under the tight budget -> (frames, budget, [the replay's result per call])"""
    w, h, K = dc.SHAPES[name]
    base = base_sequence(name)
    loose = Replay(pieces, w, h, K)
    first = [loose.call(px, 1 << 40) for px in base]
    nonkey = next(r for r in first[1:] if r["candidates"] > 0 and not r["key_frame"])
    budget = int(np.ceil(nonkey["all_bytes"] * FRACTIONS[name]))
    for _ in range(16):                                                              # raised to size(255) + 1 of every call, until that holds
        replay, results, frames = Replay(pieces, w, h, K, host), [], list(base)
        for i in range(len(base) + 32):
            if i >= len(frames):
                if results[-1]["owed"] == 0:
                    break
                frames.append(base[-1])
            r = replay.call(frames[i], budget)
            need = (replay.refused_size255 if r is None else r["size255"]) + 1
            if need > budget:
                budget = need
                break
            results.append(r)
        else:
            return frames[:len(results)], budget, results
        if len(results) >= len(base) and results[-1]["owed"] == 0 and len(results) == len(frames):
            return frames, budget, results
    raise AssertionError("no budget found")
