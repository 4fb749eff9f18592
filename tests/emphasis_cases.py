"""Emphasis maps (include/mpcodec.h, "emphasis") as a numpy model: the allocation and the sweep with a factor per tile on the distortion
term, the floor allocation with a candidate -> tile list, and the map from a pixel mask; the cases the host functions and the kernels
are held to, and the mistakes those cases must tell apart (WRONG_*: each is caught by the case CAUGHT_BY names).  Imported by
test_emphasis_cases.py (CPU) and test_gpu_emphasis.py; nothing here needs the library; budget_cases.py and rate_cases.py are used as
they are.

An allocation case is (name, profile uint32 [T, K + 1], counts uint16 [T, 3], emphasis uint8 [T], weights uint32 [3, K], js, grid) with
grid = (tiles_x, tiles_y) or None; a floor case (name, profile, counts, floor, must, emphasis uint8 [tiles], list int32 [n] or None,
weights, js); a mask case (name, buffer uint8 [rows, stride] with 255 wherever the frame is not, offset, width, height, lo, hi): the
mask is buffer.reshape(-1)[offset:] read with the buffer's stride."""
import numpy as np

import budget_cases as bc
import rate_cases as rc

NEUTRAL, E_MAX, LAMBDAS = 16, 64, bc.LAMBDAS
KS = (1, 5, 32)
TILE_COUNTS = (1, 3, 4, 5, 15, 16, 17, 33)      # across 4 waves a workgroup and 16 staged tiles
T_SWEEP_WRAP = 512 * 16 + 1                    # one past the sweep's grid cap x its chunk
T_ALLOCATE_WRAP = 4096 * 4 + 1                 # one past the allocations' grid cap x their waves

WRONG_ALLOCATE = ("e scales the rate", "factor 65536", "map read row-major", "totals[0] weighted", "0 used as 0", "above 64 not clamped",
                  "largest n on ties")
WRONG_FLOOR = ("e taken from i",)
WRONG_MASK = ("mean", "row padding read", "floor rounding", "a pixel outside the frame counts")
CAUGHT_BY = {"e scales the rate": "K5 T33 random", "factor 65536": "K5 T17 all 16", "map read row-major": "K5 T18 checkerboard 6x3",
             "totals[0] weighted": "K5 T33 random", "0 used as 0": "K5 stored 0", "above 64 not clamped": "K5 stored 255",
             "largest n on ties": "K5 flat profile", "e taken from i": "K5 listed, entries outside", "mean": "197x117 stride 210 offset 3",
             "row padding read": "9x117 stride 22 offset 3", "floor rounding": "197x117 stride 197 offset 0",
             "a pixel outside the frame counts": "197x117 stride 210 offset 3"}


def used(emphasis, mistake=None):
    e = np.asarray(emphasis, np.int64)
    if mistake != "0 used as 0":
        e = np.maximum(e, 1)
    return e if mistake == "above 64 not clamped" else np.minimum(e, E_MAX)


def _rates(counts, weights, K):
    """R[t, n] and the records kept [t, n], int64"""
    cut = np.minimum(np.asarray(counts, np.int64).reshape(-1, 3), K)
    below = np.zeros((3, K + 1), np.int64)
    below[:, 1:] = np.cumsum(np.asarray(weights, np.int64).reshape(3, K), axis=1)
    upto = np.minimum(np.arange(K + 1)[None, None, :], cut[:, :, None])
    return below[0][upto[:, 0]] + below[1][upto[:, 1]] + below[2][upto[:, 2]], upto.sum(axis=1), cut


def allocate(profile, counts, emphasis, weights, j, mistake=None, grid=None):
    """-> (depth uint8 [T], cut counts uint16 [T, 3], totals [true distortion, rate, records] as Python ints); emphasis None = neutral"""
    profile = np.asarray(profile, np.uint32)
    T, K = profile.shape[0], profile.shape[1] - 1
    R, _, cut = _rates(counts, weights, K)
    e = np.full(T, NEUTRAL, np.int64) if emphasis is None else used(emphasis, mistake)
    if mistake == "map read row-major" and grid is not None:
        tx, ty = np.divmod(np.arange(T), grid[1])
        e = e[ty * grid[0] + tx]
    L = bc.lambda_of(j)
    P = profile.astype(np.int64)
    assert T == 0 or (int(P.max()) * 255 * 65536 + L * int(R.max())) < (1 << 63), "the case leaves what int64 holds"
    if mistake == "e scales the rate":                               # beyond int64: Python ints
        J = P.astype(object) * 65536 + L * R.astype(object) * e.astype(object)[:, None]
    else:
        J = P * e[:, None] * (65536 if mistake == "factor 65536" else 4096) + L * R
    at = K - np.argmin(J[:, ::-1], axis=1) if mistake == "largest n on ties" else np.argmin(J, axis=1)
    rows = np.arange(T)
    kept = np.minimum(cut, at[:, None])
    true = P[rows, at] * e // NEUTRAL if mistake == "totals[0] weighted" else P[rows, at]
    return at.astype(np.uint8), kept.astype(np.uint16), [int(true.sum()), int(R[rows, at].sum()), int(kept.sum())]


def sweep(profile, counts, emphasis, weights, mistake=None, grid=None):
    """[[true distortion, rate, records] at j] for j = 0 ... 255"""
    return [allocate(profile, counts, emphasis, weights, j, mistake, grid)[2] for j in range(LAMBDAS)]


def allocate_floor(profile, counts, floor, must, emphasis, tile_list, weights, j, mistake=None):
    """rate_cases.allocate_floor with J = P * e * 4096 + L * R': candidate i takes emphasis[tile_list[i]] (None: i), the neutral value
    where that is outside the map; emphasis None = neutral"""
    profile = np.asarray(profile, np.uint32)
    n, K = profile.shape[0], profile.shape[1] - 1
    cut = np.minimum(np.asarray(counts, np.int64).reshape(n, 3), K)
    floor = np.zeros(n, np.int64) if floor is None else np.minimum(np.asarray(floor, np.int64), K)
    must = np.ones(n, np.int64) if must is None else np.asarray(must, np.int64)
    R = bc.rates(cut, weights, K)
    L = bc.lambda_of(j)
    depth, send, totals = np.zeros(n, np.uint8), np.zeros(n, np.uint8), [0, 0, 0, 0]
    for i in range(n):
        t = i if tile_list is None or mistake == "e taken from i" else int(tile_list[i])
        e = NEUTRAL if emphasis is None or not 0 <= t < len(emphasis) else int(used(emphasis[t]))
        low = int(floor[i])
        allowed = range(0, K + 1) if must[i] else range(low, K + 1)
        rate = {d: 0 if not must[i] and d == low else R[i, d] for d in allowed}
        J = {d: int(profile[i, d]) * e * 4096 + L * rate[d] for d in allowed}
        best = min(J.values())
        depth[i] = next(d for d in allowed if J[d] == best)
        send[i] = 1 if must[i] or depth[i] > low else 0
        totals[0] += int(profile[i, depth[i]])
        totals[1] += rate[int(depth[i])]
        if send[i]:
            totals[2] += int(np.minimum(cut[i], int(depth[i])).sum())
            totals[3] += 1
    return depth, np.minimum(cut, depth[:, None].astype(np.int64)).astype(np.uint16), send, totals


def mask_view(buffer, offset, width, height):
    """the mask of a case as a numpy view [height, width] into its buffer: nothing is copied, the stride and the odd base are kept"""
    stride = buffer.shape[1]
    flat = buffer.reshape(-1)
    return np.lib.stride_tricks.as_strided(flat[offset:], (height, width), (stride, 1), writeable=False)


def from_mask(buffer, offset, width, height, lo, hi, mistake=None):
    """-> emphasis uint8 [tiles], t = tx * tiles_y + ty"""
    stride = buffer.shape[1]
    flat = buffer.reshape(-1).astype(np.int64)
    tiles_x, tiles_y = -(-width // 8), -(-height // 8)
    out = np.zeros(tiles_x * tiles_y, np.uint8)
    for tx in range(tiles_x):
        for ty in range(tiles_y):
            x1 = min(tx * 8 + 8, stride) if mistake == "row padding read" else min(tx * 8 + 8, width)
            y1 = min(ty * 8 + 8, height)
            if mistake == "a pixel outside the frame counts":
                y1 = min(ty * 8 + 8, (flat.size - offset) // stride)         # the rows the buffer holds under the frame
            v = np.array([flat[offset + y * stride + x] for y in range(ty * 8, y1) for x in range(tx * 8, x1)])
            m = int(v.sum()) // v.size if mistake == "mean" else int(v.max())
            out[tx * tiles_y + ty] = lo + ((hi - lo) * m + (0 if mistake == "floor rounding" else 127)) // 255
    return out


# ---- the cases ----
def _random_map(rng, T):
    e = rng.integers(1, E_MAX + 1, T).astype(np.uint8)
    e[rng.random(T) < 0.1] = 0                                       # used as 1
    e[rng.random(T) < 0.1] = 255                                     # used as 64
    e[rng.random(T) < 0.2] = NEUTRAL
    return e


def _random_case(rng, K, T, label="random"):
    counts = rng.integers(0, K + 2, (T, 3)).astype(np.uint16)        # K + 1: a count above K
    if T > 1:
        counts[1] = (65535, 0, K)
    P = bc._consistent_profile(rng, np.minimum(counts, K), K, monotone=False)
    return (f"K{K} T{T} {label}", P, counts, _random_map(rng, T), bc._weights(rng, K, "extreme"), (0, 1, 60, 113, 160, 255), None)


def _falling(K, T, start, step):
    return np.maximum(start - step * np.arange(K + 1, dtype=np.int64), 0)[None, :].repeat(T, 0).astype(np.uint32)


def cases(large=False):
    """Every profile stays within P_MAX = 12 484 800 < 2^24, which the sweep kernel's staged entry relies on.  large: also the tile counts that wrap the kernels' grids (for the device; the model is not run on them)"""
    rng = np.random.default_rng(20241021)
    out = []
    for K in KS:
        for T in TILE_COUNTS:
            out.append(_random_case(rng, K, T))
        T = 17
        name, P, counts, _, W, js, _ = _random_case(rng, K, T)
        for value in (1, NEUTRAL, E_MAX):
            out.append((f"K{K} T{T} all {value}", P, counts, np.full(T, value, np.uint8), W, js, None))
        # at the bound: the largest profile under the largest factor at the largest multiplier still keeps nothing
        full = np.full((T, 3), K, np.uint16)
        P = np.full((T, K + 1), bc.P_MAX, np.uint32)
        P[:, 1:] = 0
        out.append((f"K{K} at the bound", P, full, np.where(np.arange(T) % 2, 255, E_MAX).astype(np.uint8), np.full((3, K), bc.W_MIN, np.uint32),
                    (255, 254, 200), None))
        # a checkerboard in tile coordinates on a grid with tiles_x != tiles_y: 64 where tx + ty is odd, 1 elsewhere, x outer.  6 x 3, not
        # 5 x 3: with both sides odd t = tx * tiles_y + ty and ty * tiles_x + tx have the parity of tx + ty, and the board reads the same
        tx, ty = np.divmod(np.arange(18), 3)
        out.append((f"K{K} T18 checkerboard 6x3", _falling(K, 18, 2_000_000, 50_000) + rng.integers(0, 1000, (18, K + 1)).astype(np.uint32),
                    np.full((18, 3), K, np.uint16), np.where((tx + ty) % 2, E_MAX, 1).astype(np.uint8), np.full((3, K), 1000, np.uint32),
                    (100, 113, 120, 130), (6, 3)))
        T = 6
        full = np.full((T, 3), K, np.uint16)
        flat_w = np.full((3, K), 1000, np.uint32)
        # a flat profile: every depth ties at j = 0, and beyond the counts at any j
        out.append((f"K{K} flat profile", np.full((T, K + 1), 77777, np.uint32), full, _random_map(rng, T), flat_w, (0, 1, 255), None))
        # stored 0 is 1, not 0: at L = 8 a step costs 8 * 3000, and falls P by 300 000 * 4096
        out.append((f"K{K} stored 0", _falling(K, T, 12_000_000, 300_000), full, np.zeros(T, np.uint8), flat_w, (1, 2), None))
        # stored 255 is 64: at L = 8 << 14 a step costs 3.9e8, between 64 * 4096 * 1000 = 2.6e8 and 255 * 4096 * 1000 = 1.0e9
        out.append((f"K{K} stored 255", _falling(K, T, 100_000, 1000), full, np.full(T, 255, np.uint8), flat_w, (1 + 8 * 14,), None))
    if large:
        for K, T in ((1, T_ALLOCATE_WRAP), (5, T_SWEEP_WRAP), (32, T_SWEEP_WRAP)):
            out.append(_random_case(rng, K, T, "wraps"))
    return out


def floor_cases(large=False):
    rng = np.random.default_rng(20241022)
    out = []
    for K in KS:
        for n in TILE_COUNTS + ((T_ALLOCATE_WRAP,) if large and K == 5 else ()):
            _, P, counts, _, W, js, _ = _random_case(rng, K, n)
            tiles = n + 7
            e = _random_map(rng, tiles)
            full = rc.full_depth(counts, K)
            floor = np.where(rng.random(n) < 0.5, full // 2, rng.integers(0, K + 3, n)).astype(np.uint8)
            must = (rng.random(n) < 0.4).astype(np.uint8)
            listed = np.sort(rng.choice(tiles, n, replace=False)).astype(np.int32)
            outside = listed.copy()
            outside[::3] = np.array([-1, tiles, 2**31 - 1, -2**31])[np.arange(len(outside[::3])) % 4]
            out.append((f"K{K} n{n} no list", P, counts, floor, must, e[:n], None, W, js))
            out.append((f"K{K} n{n} listed", P, counts, floor, must, e, listed, W, js))
            out.append((f"K{K} n{n} listed, must and floor null", P, counts, None, None, e, listed, W, js))
            if n == 33:
                out.append((f"K{K} listed, entries outside", P, counts, floor, must, e, outside, W, js))
    return out


MASK_WIDTHS, MASK_HEIGHTS = (1, 7, 8, 9, 197), (1, 117)


def _mask_case(rng, width, height, stride, offset, lo, hi, below=0):
    """the frame's bytes random (half of them 0, so that a tile's maximum varies), 255 in the row padding, in front of the odd base and in
    `below` rows under the frame"""
    rows = height + below + 1
    buffer = np.full((rows, stride), 255, np.uint8)
    body = rng.integers(0, 256, (height, width)).astype(np.uint8)
    body[rng.random((height, width)) < 0.5] = 0
    body[rng.random((height, width)) < 0.3] //= 16
    flat = buffer.reshape(-1)
    for y in range(height):
        flat[offset + y * stride:offset + y * stride + width] = body[y]
    return (f"{width}x{height} stride {stride} offset {offset}", buffer, offset, width, height, lo, hi)


def mask_cases(wide=False):
    rng = np.random.default_rng(20241023)
    out = []
    for width in MASK_WIDTHS:
        for height in MASK_HEIGHTS:
            out.append(_mask_case(rng, width, height, width, 0, 1, E_MAX))
            out.append(_mask_case(rng, width, height, width + 13, (1, 3)[width % 2], 4, E_MAX, below=9))
    out.append(_mask_case(rng, 197, 117, 200, 0, NEUTRAL, NEUTRAL))
    out.append(_mask_case(rng, 64, 48, 64, 0, 8, 40))
    # a base and a stride that are multiples of 4 (the kernel then loads four pixels at once) under widths that are not
    for width, stride, offset in ((1, 4, 0), (7, 20, 0), (9, 12, 4), (197, 200, 8)):
        out.append(_mask_case(rng, width, 117, stride, offset, 1, E_MAX, below=3))
    if wide:
        out.append(_mask_case(rng, 4928, 8, 4928, 0, 1, E_MAX))       # a single tile row, 616 tiles: many workgroups across
        out.append(_mask_case(rng, 4928, 5, 4931, 1, 1, E_MAX))
    return out


# ---- the session's replay with a map ----
class Replay(rc.Replay):
    """rate_cases.Replay with an emphasis map: the same call, its floor allocation replaced by allocate_floor above for the length of
    the call -- the candidates are worked out here as the call works them out, since the allocation needs candidate -> tile."""
    emphasis = None

    def call(self, px, budget, key=False):
        if self.emphasis is None:
            return super().call(px, budget, key)
        is_key = key or self.sent is None or self.kept is None
        if is_key:
            cand = None
        else:
            counts, _ = self.p.records(px)
            cand = rc.owed_tiles(self.sent, counts, self.K, rc.dc.changed_tiles(self.kept, px))[0]
        e, plain, host = self.emphasis, rc.allocate_floor, self.host
        rc.allocate_floor = lambda P, c, f, m, w, j: allocate_floor(P, c, f, m, e, cand, w, j)
        self.host = None                                             # the host's plain allocation is not this one
        try:
            return super().call(px, budget, key)
        finally:
            rc.allocate_floor, self.host = plain, host


def central_map(width, height, inside=E_MAX, outside=4):
    """the end-to-end tests' map: a central rectangle of tiles at `inside` over `outside`"""
    tiles_x, tiles_y = -(-width // 8), -(-height // 8)
    tx, ty = np.divmod(np.arange(tiles_x * tiles_y), tiles_y)
    centre = (tx >= tiles_x // 4) & (tx < tiles_x - tiles_x // 4) & (ty >= tiles_y // 4) & (ty < tiles_y - tiles_y // 4)
    return np.where(centre, inside, outside).astype(np.uint8)
