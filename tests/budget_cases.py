"""The rate control of mpc_encode_image_budget as a numpy model (include/mpcodec.h, "budget"), the cases the host function and the
allocation kernel are held to, and the mistakes those cases must tell apart.  Imported by test_budget_cases.py (CPU) and
test_gpu_budget.py; nothing here needs the library.

A case is (name, profile uint32 [T, K + 1], counts uint16 [T, 3], weights uint32 [3, K], js).  Profiles stay below 2^24 (64 pixels of
3 * 255^2) and weights inside the clamp 256 ... 2^20, as the contract bounds them."""
import numpy as np

LAMBDAS = 256
W_MIN, W_MAX = 256, 1 << 20
P_MAX = 64 * 3 * 255 * 255


def lambda_of(j):
    return 0 if j == 0 else (8 + (j - 1) % 8) << ((j - 1) // 8)


def weights_from_streams(streams, K, clamp=True):
    """streams: per stream of the 1 + 6K a dict with wrapper_bit, end_bit, expect (api.index_info's) -> W uint32 [3, K] (object ints
    without the clamp)"""
    W = np.zeros((3, K), object)
    for ch in range(3):
        for i in range(K):
            a = 1 + 2 * K * ch + 2 * i
            bits, n = int(streams[a + 1]["end_bit"]) - int(streams[a]["wrapper_bit"]), int(streams[a]["expect"])
            w = W_MIN if n == 0 else (256 * bits + n // 2) // n
            W[ch, i] = min(max(w, W_MIN), W_MAX) if clamp and n else w
    return W.astype(np.uint32) if clamp else W


def rates(counts, weights, K, mistake=None):
    """R[t, n] as Python ints (object array [T, K + 1])"""
    counts = np.minimum(np.asarray(counts, np.int64), K)
    below = np.zeros((3, K + 1), object)
    for ch in range(3):
        src = 0 if mistake == "one channel's weights" else ch
        for i in range(K):
            below[ch, i + 1] = below[ch, i] + int(weights[src, i])
    R = np.zeros((counts.shape[0], K + 1), object)
    for t in range(counts.shape[0]):
        for n in range(K + 1):
            R[t, n] = sum(below[ch, n if mistake == "rate without min" else min(n, int(counts[t, ch]))] for ch in range(3))
    return R


def allocate(profile, counts, weights, j, mistake=None):
    """-> (depth uint8 [T], cut counts uint16 [T, 3], totals [distortion, rate, records] as Python ints); mistake: None or one of WRONG"""
    profile = np.asarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    counts = np.minimum(np.asarray(counts, np.int64).reshape(T, 3), K)
    R = rates(counts, weights, K, mistake)
    L = lambda_of(j)
    scale = 1 if mistake == "scale dropped" else 65536
    depth = np.zeros(T, np.uint8)
    totals = [0, 0, 0]
    for t in range(T):
        J = [int(profile[t, n]) * scale + L * R[t, n] for n in range(K + 1)]
        best = min(J)
        at = [n for n in range(K + 1) if J[n] == best]
        depth[t] = at[-1] if mistake == "largest n on ties" else at[0]
        totals[0] += int(profile[t, depth[t]])
        totals[1] += R[t, depth[t]]
    cut = np.minimum(counts, depth[:, None].astype(np.int64)).astype(np.uint16)
    totals[2] = int(counts.sum()) if mistake == "totals from the uncut counts" else int(cut.sum())
    return depth, cut, totals


WRONG = ("largest n on ties", "rate without min", "one channel's weights", "scale dropped", "totals from the uncut counts")
WRONG_WEIGHTS = ("no clamp",)


def _consistent_profile(rng, counts, K, monotone=True):
    """a profile as the kernel makes one: depths above a tile's largest count repeat the last value"""
    T = counts.shape[0]
    P = np.zeros((T, K + 1), np.uint32)
    for t in range(T):
        deepest = min(int(counts[t].max()), K)
        v = int(rng.integers(1000, P_MAX))
        P[t, 0] = v
        for n in range(1, K + 1):
            if n <= deepest:
                v = max(0, v - int(rng.integers(0, v // 2 + 2))) if monotone or rng.random() < 0.7 else min(P_MAX, v + int(rng.integers(1, 5000)))
            P[t, n] = v
    return P


def _weights(rng, K, kind="mixed"):
    if kind == "flat":
        return np.full((3, K), 1000, np.uint32)
    W = rng.integers(W_MIN, 20000, (3, K)).astype(np.uint32)
    W[1] //= 3                                           # the chroma channels cost less: one channel's weights for all must show
    W[2] //= 5
    W = np.maximum(W, W_MIN)
    if kind == "extreme":
        W[0, 0], W[2, K - 1] = W_MAX, W_MIN
    return W


def cases():
    rng = np.random.default_rng(20240917)
    out = []
    js_all = (0, 1, 40, 90, 120, 160, 200, 255)
    for K in (1, 8, 32):
        for T in (1, 63, 64, 65):
            counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)          # counts that differ by channel
            counts[rng.random(T) < 0.15] = 0                                  # tiles whose three counts are all 0
            out.append((f"K{K} T{T} monotone", _consistent_profile(rng, counts, K), counts, _weights(rng, K), js_all))
            out.append((f"K{K} T{T} not monotone", _consistent_profile(rng, counts, K, monotone=False), counts, _weights(rng, K, "extreme"), js_all))
    # the grid stride: more tiles than one launch's waves take in one round is beyond a test; more than a workgroup's is not
    K, T = 8, 4097
    counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
    out.append(("K8 T4097", _consistent_profile(rng, counts, K, monotone=False), counts, _weights(rng, K), (0, 100, 150, 255)))
    # equal J at several depths: a flat profile at j = 0 and beyond the counts, and exact ties at L > 0: P falls by L * w / 65536 a step
    for K in (8, 32):
        T = 65
        counts = np.full((T, 3), K, np.uint16)
        counts[::3, 1] = K // 2
        counts[1::5] = 0
        P = np.full((T, K + 1), 77777, np.uint32)
        out.append((f"K{K} flat profile", P, counts, _weights(rng, K, "flat"), (0, 1, 255)))
        j = 1 + 8 * 16                                                       # L = 8 << 16: L * 3000 / 65536 = 24000 exactly
        W = np.full((3, K), 1000, np.uint32)
        full = np.full((T, 3), K, np.uint16)
        P = (2_000_000 - 24000 * np.arange(K + 1, dtype=np.int64))[None, :].repeat(T, 0).astype(np.uint32)
        out.append((f"K{K} exact ties", P, full, W, (j, j - 1, j + 1)))
    # a count above K is used as K
    K, T = 8, 64
    counts = rng.integers(0, K + 1, (T, 3)).astype(np.uint16)
    counts[5, 1], counts[17, 2] = K + 1, 65535
    out.append(("K8 counts above K", _consistent_profile(rng, np.minimum(counts, K), K), counts, _weights(rng, K), (0, 60, 130, 255)))
    return out


def damaged_indexes(index):
    """(label, blob): a seek index cut short, with a wrong magic, empty, and with single bits flipped through its header and stream records"""
    index = bytes(index)
    out = [("empty", b""), ("one byte", index[:1]), ("cut in the header", index[:20]), ("cut in the streams", index[:len(index) // 2]),
           ("one byte short", index[:-1]), ("wrong magic", bytes([index[0] ^ 0xFF]) + index[1:])]
    rng = np.random.default_rng(7)
    for k in range(40):
        at = int(rng.integers(0, min(len(index), 4096)))
        b = bytearray(index)
        b[at] ^= 1 << int(rng.integers(0, 8))
        out.append((f"bit flip at {at}", bytes(b)))
    return out
