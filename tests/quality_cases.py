"""The target-quality encode of mpc_encode_image_quality as a numpy model (include/mpcodec.h, "quality"): the sweep -- the allocation's
three totals at all 256 multipliers -- and the pick, the cases the host functions and the sweep kernel are held to, and the mistakes
those cases must tell apart.  Imported by test_quality_cases.py (CPU) and test_gpu_target_quality.py; nothing here needs the library, and
budget_cases.py is used as it is.

The sweep is budget_cases.allocate at each j (`sweep_by_allocate`, a Python loop per tile); `sweep` is the same in vectorised uint64
arithmetic -- J stays below 2^64 for a profile and weights inside their bounds -- and test_quality_cases.py holds the two to each
other.  A case is (name, profile uint32 [T, K + 1], counts uint16 [T, 3], weights uint32 [3, K])."""
import numpy as np

import budget_cases as bc

LAMBDAS = bc.LAMBDAS
U64_MAX = (1 << 64) - 1

WRONG_SWEEP = ("largest n on ties", "multiplier of j + 1", "u32 totals", "records from the uncut counts")
WRONG_PICK = ("smallest j", "strict <", "bisect on the rate total")


def sweep_by_allocate(profile, counts, weights, js=range(LAMBDAS)):
    """{j: [distortion, rate, records]} from budget_cases.allocate, Python ints"""
    return {j: [int(v) for v in bc.allocate(profile, counts, weights, j)[2]] for j in js}


def sweep(profile, counts, weights, mistake=None):
    """S[j] = [distortion, rate in 1/256 bit, records kept] at multiplier j = 0 ... 255, as a list of lists of Python ints"""
    profile = np.asarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    cut = np.minimum(np.asarray(counts, np.int64).reshape(T, 3), K)
    below = np.zeros((3, K + 1), np.uint64)
    below[:, 1:] = np.cumsum(np.asarray(weights, np.uint64).reshape(3, K), axis=1)
    n = np.arange(K + 1, dtype=np.int64)
    upto = np.minimum(n[None, None, :], cut[:, :, None])                     # [T, 3, K + 1]
    R = (below[0][upto[:, 0, :]] + below[1][upto[:, 1, :]] + below[2][upto[:, 2, :]]).astype(np.uint64)
    kept = upto.sum(axis=1)                                                  # [T, K + 1]
    P16 = profile.astype(np.uint64) << np.uint64(16)
    rows = np.arange(T)
    out = []
    for j in range(LAMBDAS):
        L = bc.lambda_of(j + 1 if mistake == "multiplier of j + 1" else j)      # the formula holds one entry beyond the table
        assert T == 0 or int(P16.max()) + L * int(R.max()) <= U64_MAX, "the case leaves the bounds the u64 arithmetic is exact in"
        J = P16 + np.uint64(L) * R
        at = K - np.argmin(J[:, ::-1], axis=1) if mistake == "largest n on ties" else np.argmin(J, axis=1)     # argmin: the first minimum
        totals = [sum(int(v) for v in profile[rows, at]), sum(int(v) for v in R[rows, at]),
                  int(cut.sum()) if mistake == "records from the uncut counts" else int(kept[rows, at].sum())]
        out.append([v & 0xFFFFFFFF for v in totals] if mistake == "u32 totals" else totals)
    return out


def pick(S, max_sse, mistake=None):
    """the largest j with S[j][0] <= max_sse, -1 if there is none"""
    if mistake == "bisect on the rate total":
        lo, hi = -1, LAMBDAS
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if S[mid][1] <= max_sse:
                lo = mid
            else:
                hi = mid
        return lo
    ok = [j for j in range(LAMBDAS) if (S[j][0] < max_sse if mistake == "strict <" else S[j][0] <= max_sse)]
    if not ok:
        return -1
    return ok[0] if mistake == "smallest j" else ok[-1]


def pick_targets(S):
    """the targets the pick is tested at: every D[j] and the value below it, 0, D[0] - 1 and 2^64 - 1"""
    out = {0, U64_MAX}
    for j in range(LAMBDAS):
        out.add(S[j][0])
        if S[j][0] > 0:
            out.add(S[j][0] - 1)
    return sorted(out)


# ---- the frames of the end-to-end tests, and what tests/golden/budget_bytes_parent.json records of them ----
# (name, width, height, seed of the oracle's synth_frame): the stream-contract tests' frame with its partial right column and bottom
# row, and a frame of whole tiles
FRAMES = (("ragged", 197, 117, 101), ("whole", 64, 48, 77))
FRAME_KS = (8, 32)
BUDGET_QUARTERS = (4, 3, 2)                  # budgets of this many quarters of the full container's length


def budget_golden_key(frame, K, fast, quarters):
    return f"{frame} K{K} {'fast' if fast else 'double'} {quarters}/4"


def budget_golden(context, synth_frame, hashlib):
    """{key: what mpc_encode_image_budget returns for it}: the budget encode of every frame, K, flavour and budget, with the full
    container's length and hash beside it; context(K, fast) -> a device context at quality 3.5.  tools/record_budget_hashes.py wrote
    tests/golden/budget_bytes_parent.json with it from the commit in front of the target-quality encode; test_gpu_target_quality.py compares."""
    out = {}
    for name, W, H, seed in FRAMES:
        rgb = synth_frame(W, H, seed)
        for K in FRAME_KS:
            for fast in (False, True):
                ctx = context(K, fast)
                full = ctx.encode_image(rgb)
                for quarters in BUDGET_QUARTERS:
                    try:
                        got = ctx.encode_image_budget(rgb, len(full) * quarters // 4, index_interval=0)
                    except RuntimeError as e:                        # a budget below the smallest container: the refusal is the result
                        out[budget_golden_key(name, K, fast, quarters)] = dict(full_bytes=len(full), refused=str(e))
                        continue
                    out[budget_golden_key(name, K, fast, quarters)] = dict(
                        full_bytes=len(full), full_sha256=hashlib.sha256(full).hexdigest(), size=len(got.container),
                        sha256=hashlib.sha256(got.container).hexdigest(), index_sha256=hashlib.sha256(got.index).hexdigest(),
                        depth_sha256=hashlib.sha256(got.depth.tobytes()).hexdigest(), lambda_index=got.lambda_index, probes=got.probes,
                        sse=got.sse, records=got.records)
    return out


# ---- what tests/golden/cut_bytes_parent.json records of the same frames: the other routes through the cut encodes' front end ----
QUALITY_MULTIPLES = (1, 2, 4)                # targets of this many times the full frame's squared error
EMPHASIS_QUARTERS = (3, 2)                   # budgets of the encodes with an emphasis map
EMPHASIS_MULTIPLE = 2                        # ... and their quality target
STREAM_FRAMES = 3                            # calls of the delta stream: a key frame, a quarter changed, the same frame again


def emphasis_map(tiles):
    return ((7 * np.arange(tiles)) % 64 + 1).astype(np.uint8)


def stream_frames(synth_frame, W, H, seed):
    """a frame, the same with the top left quarter from another, and that one again: its owed tiles are refined"""
    first = synth_frame(W, H, seed)
    second = first.copy()
    second[:H // 2, :W // 2] = synth_frame(W, H, seed + 1)[:H // 2, :W // 2]
    return first, second, second


def _cut_entry(hashlib, got, fields):
    out = dict(size=len(got.container), sha256=hashlib.sha256(got.container).hexdigest(), index_sha256=hashlib.sha256(got.index).hexdigest(),
               depth_sha256=hashlib.sha256(got.depth.tobytes()).hexdigest())
    out.update({f: getattr(got, f) for f in fields})
    return out


def cut_golden(context, synth_frame, hashlib, to_device):
    """{key: what the call returns, or the refusal's message}: mpc_encode_image_quality at QUALITY_MULTIPLES of the full frame's error and
    one target below the best a cut reaches; the budget and the quality encode with emphasis_map, host form and device form; and
    DeltaEncoder.encode_patch_budget over stream_frames at half the first frame's full container.  to_device(array) -> a device tensor
    holding it, ready to be read on any stream.  tools/record_budget_hashes.py --all wrote tests/golden/cut_bytes_parent.json with it from
    the commit in front of the shared front end; test_gpu_target_quality.py compares."""
    quality = ("lambda_index", "sse", "records", "model_bits_256")
    budget = ("lambda_index", "probes", "sse", "records")
    out = {}

    def record(key, call):
        try:
            out[key] = call()
        except RuntimeError as e:
            out[key] = dict(refused=str(e))

    for name, W, H, seed in FRAMES:
        rgb = synth_frame(W, H, seed)
        tiles = -(-W // 8) * -(-H // 8)
        emphasis = emphasis_map(tiles)
        d_rgb, d_emphasis = to_device(rgb), to_device(emphasis)
        for K in FRAME_KS:
            for fast in (False, True):
                ctx = context(K, fast)
                head = f"{name} K{K} {'fast' if fast else 'double'}"
                full = ctx.encode_image(rgb)
                loosest = ctx.encode_image_quality(rgb, max_sse=U64_MAX // 2)
                for m in QUALITY_MULTIPLES:
                    record(f"{head} quality x{m}",
                           lambda: _cut_entry(hashlib, ctx.encode_image_quality(rgb, max_sse=loosest.full_sse * m, index_interval=0), quality))
                if loosest.min_sse > 0:
                    record(f"{head} quality below the best", lambda: _cut_entry(hashlib, ctx.encode_image_quality(rgb, max_sse=loosest.min_sse - 1), quality))
                for quarters in EMPHASIS_QUARTERS:
                    size = len(full) * quarters // 4
                    record(f"{head} emphasis budget {quarters}/4 host",
                           lambda: _cut_entry(hashlib, ctx.encode_image_budget_emphasis(rgb, size, emphasis, index_interval=0), budget))
                    record(f"{head} emphasis budget {quarters}/4 device",
                           lambda: _cut_entry(hashlib, ctx.encode_image_budget_emphasis_device(d_rgb.data_ptr(), W, H, size, d_emphasis.data_ptr(),
                                                                                               index_interval=0), budget))
                target = loosest.full_sse * EMPHASIS_MULTIPLE
                record(f"{head} emphasis quality x{EMPHASIS_MULTIPLE} host",
                       lambda: _cut_entry(hashlib, ctx.encode_image_quality_emphasis(rgb, emphasis, max_sse=target, index_interval=0), quality))
                record(f"{head} emphasis quality x{EMPHASIS_MULTIPLE} device",
                       lambda: _cut_entry(hashlib, ctx.encode_image_quality_emphasis_device(d_rgb.data_ptr(), W, H, d_emphasis.data_ptr(), max_sse=target,
                                                                                            index_interval=0), quality))
                session = ctx.delta_encoder(W, H)
                for k, frame in enumerate(stream_frames(synth_frame, W, H, seed)):
                    def call():
                        patch, info = session.encode_patch_budget(frame, len(full) // 2)
                        entry = dict(size=len(patch), sha256=hashlib.sha256(patch).hexdigest(), sent_sha256=hashlib.sha256(session.sent().tobytes()).hexdigest())
                        entry.update({f: getattr(info, f) for f in info.__slots__})
                        return entry
                    record(f"{head} stream {k}", call)
                session.close()
    return out


def cases():
    out = [(name, P, counts, W) for name, P, counts, W, _js in bc.cases()]
    rng = np.random.default_rng(20241020)
    # few tiles, and one more than a workgroup's chunk of them holds many times over; profiles not monotone in depth; counts 0 and K + 1
    for K in (1, 8, 32):
        for T in (1, 3, 4, 5, 257):
            counts = rng.integers(0, K + 2, (T, 3)).astype(np.uint16)
            counts[0] = (K + 1, 0, K)
            if T > 1:
                counts[1] = 0
            P = bc._consistent_profile(rng, np.minimum(counts, K), K, monotone=False)
            out.append((f"K{K} T{T} quality", P, counts, bc._weights(rng, K, "extreme")))
    # the largest J there is: P_MAX beside the largest rate at the largest multiplier, 14 * 2^31 * 96 * 2^20 < 2^62
    K, T = 32, 5
    counts = np.full((T, 3), K, np.uint16)
    counts[3] = (K + 1, 65535, K)
    P = np.full((T, K + 1), bc.P_MAX, np.uint32)
    P[1] = np.linspace(bc.P_MAX, 0, K + 1).astype(np.uint32)
    P[2, 1::2] = bc.P_MAX - 1
    out.append(("K32 largest J", P, counts, np.full((3, K), bc.W_MAX, np.uint32)))
    # a distortion total above 2^32: 400 tiles near P_MAX at depth 0
    K, T = 1, 400
    counts = rng.integers(0, K + 2, (T, 3)).astype(np.uint16)
    P = np.zeros((T, K + 1), np.uint32)
    P[:, 0] = bc.P_MAX - rng.integers(0, 1000, T)
    P[:, 1] = np.where(counts.max(axis=1) > 0, rng.integers(0, 5_000_000, T), P[:, 0])
    out.append(("K1 T400 above 2^32", P, counts, bc._weights(rng, K)))
    return out
