"""Inputs of the pursuit-kernel parity tests, shared by the double flavour (test_gpu_parity.py), the float flavour
(test_gpu_fast_parity.py), the CPU check of the inputs themselves (test_pursuit_cases.py) and tools/fuzz_parity.py.

Vector classes (`vector_classes`): 64-vectors for matching::CalcMPDynamic[Fast].  Every class runs in two FORMS:
  "table"  the context's own quantiser tables (the screen's thresholds as a frame sees them);
  "tiny"   one step `tiny_quant(v)` for all K steps, far below the data: the pursuit stays alive for all K steps and the
           residual shrinks to rounding noise.  This is the form in which float and double arithmetic give different records.

WELL-DEFINEDNESS is a condition on the input, not a tolerance on the result.  The reference has undefined behaviour where
round(best / quant) leaves the int range and where a float intermediate overflows; a case is kept for the float flavour only if
  * every input is finite as f32 (class "nan" excepted, see below), and
  * "table": max|v| < 1e6.  The dictionary rows have unit norm, so |best| <= 8 max|v| < 8e6 and the tables hold no step
    below 1.0: |best / quant| < 2^23.
  * "tiny":  max|v| <= 1e37, so that 8 max|v| (the bound of every partial sum of a projection and of every residual) is finite
    in f32; the step is q = max(max|v| * 2^-20, 2^-126): a normal, non-zero f32 after the cast (a smaller q casts to a
    subnormal or to 0.0f, and best / 0.0f is the undefined conversion again), and |best / q| <= 8 * 2^20.
Class "nan": a NaN anywhere in the input makes every projection NaN (each is a sum over all 64 elements), `fabsf(p) > -1` is
false for every row, the index stays -1 and the pursuit ends before anything is divided or converted: defined, whatever the
other elements are, as long as they are finite or NaN.
`well_defined` returns the kept AND the rejected cases with the reason; test_pursuit_cases.py holds the exact counts.
The double flavour keeps its own, wider rules (test_gpu_parity.py: < 1e6 with the tables, < 1e100 with the tiny step)."""
import numpy as np

F32_MIN_NORMAL = 2.0 ** -126
FORMS = ("table", "tiny")
TABLE_LIMIT = 1e6
TINY_LIMIT = 1e37
CANNOT_SEPARATE = ("zero_and_sign", "nan")     # no arithmetic happens that could tell float from double


# ---- the double tests' builders, moved here unchanged ------------------------------------------------------------------

def adversarial_vectors():
    """Inputs that stress the filter's threshold logic: exact ties (mirror-symmetric and constant tiles), magnitudes from
    the f32 subnormal range to beyond the f32 range, impulses, residuals that are rounding noise after the DC atom."""
    rng = np.random.default_rng(2024)
    v = []
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    for f in (x, y, x + y, x - y, (x - 3.5) ** 2, np.abs(x - 3.5) + np.abs(y - 3.5), (x ^ y) & 1, (x // 4) * 2 + (y // 4)):
        v.append(f.reshape(-1).astype(np.float64) * 17.0)                       # symmetric patterns: exact ties
        v.append(f.T.reshape(-1).astype(np.float64) * 17.0 + 3.0)
    for c in (1.0, 128.0, 255.0, 0.1, 1e-3):
        v.append(np.full(64, c))                                               # flat: residual after DC is rounding noise
    for k in (0, 7, 27, 63):
        e = np.zeros(64); e[k] = 200.0; v.append(e)                             # impulses
    base = rng.integers(0, 256, (6, 64)).astype(np.float64)
    for scale in (1e-300, 1e-160, 1e-45, 1e-38, 1e-30, 1e-10, 1.0, 1e10, 1e30, 1e38, 1e39, 1e150, 1e300):
        v.extend(list(base * scale))                                           # f32 under/overflow on the filter side
    v.extend(list(rng.standard_normal((40, 64)) * 1e-20))
    v.append(np.zeros(64))
    return np.array(v)


def near_tie_vectors(base):
    """Residuals built as equal-weight sums of several adjacent base rows (three or more rows inside the filter window at once),
    each next to a clear neighbour.  base: the dictionary's base rows [510, 64]."""
    rng = np.random.default_rng(123)
    v = []
    for rep in range(48):
        r0 = int(rng.integers(1, 500))
        picks = [r0, r0 + 1, r0 + 2, r0 + 3, r0 + 4][: 3 + rep % 3]         # adjacent rows: the four rows of one lane
        w = sum(base[p] for p in picks) * 300.0
        v.append(w)
        v.append(rng.integers(0, 256, 64).astype(np.float64))               # a clear neighbour
    return np.array(v)


NAN_ROWS = 5      # the first rows of nan_vectors() hold a NaN, the others are clean neighbours


def nan_vectors():
    rng = np.random.default_rng(77)
    v = rng.integers(0, 256, (12, 64)).astype(np.float64)
    v[0, :] = np.nan
    v[1, 0] = np.nan
    v[2, 63] = np.nan
    v[3, 17] = -np.nan
    v[4, ::2] = np.nan
    return v


def degenerate_frames(K):
    """Flat frames (black: every residual is zero from the start; white and grey: only the DC atom matters), one-pixel
    checkerboards and stripes (energy in the highest frequencies), hard 0/255 noise, a 1x1 image and a single column."""
    H, W = 24, 40
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(K)
    frames = {
        "black": np.zeros((H, W, 3), np.uint8),
        "white": np.full((H, W, 3), 255, np.uint8),
        "grey": np.full((H, W, 3), 128, np.uint8),
        "checker": np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2),
        "stripes": np.stack([((xx & 1) * 255), ((yy & 1) * 255), (((xx >> 2) & 1) * 255)], axis=2).astype(np.uint8),
        "hard noise": (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8),
        "one pixel": np.array([[[200, 30, 90]]], np.uint8),
        "one column": rng.integers(0, 256, (19, 1, 3)).astype(np.uint8),
    }
    return {name: np.ascontiguousarray(rgb) for name, rgb in frames.items()}


# ---- float-only classes ------------------------------------------------------------------------------------------------

def _pixel_base():
    return np.random.default_rng(31).integers(0, 256, (6, 64)).astype(np.float64)


def f32_subnormal_inputs(base):
    """(a) every non-zero input is an f32 subnormal: the pixel vectors scaled (255 * 4e-41 < 2^-126), and base rows times
    1.5 and 2.5 steps of the tiny form (q = 2^-126 there; the first six rows whose entries all stay below 0.39, so that
    2.5 q |entry| < q), whose step-0 projection lies at a rounding boundary of round(best / q) up to the rounding of
    subnormal products."""
    v = [_pixel_base() * s for s in (1e-45, 1e-43, 1e-41, 4e-41)]
    rows = [r for r in range(1, base.shape[0]) if np.abs(base[r]).max() < 0.39][:6]
    v.append(np.array([base[r] * (c * F32_MIN_NORMAL) for r in rows for c in (1.5, 2.5)]))
    return np.vstack(v)


def f32_subnormal_products():
    """(b) inputs are normal f32 numbers (or zero), their products with the dictionary's small entries (1e-3 and below) are
    subnormal."""
    return np.vstack([_pixel_base() * s for s in (3e-37, 1e-36, 3e-36, 1e-35)])


def f32_subnormal_residuals():
    """(c) normal inputs whose residual reaches the subnormal range only after some steps of the tiny-quant recipe: the pixel
    vectors with one pixel unit just above 2^-126 = 1.18e-38 (the step is clamped to 2^-126: residual elements below one
    unit are subnormal), and the symmetric patterns and flat tiles of adversarial_vectors() around max|v| = 2^20 * 2^-126
    (few atoms describe them, so the residual falls from 2^20 steps to below one step, i.e. into the subnormal range,
    while the step is still the recipe's max|v| * 2^-20)."""
    return np.vstack([_pixel_base() * s for s in (1.2e-38, 2e-38, 5e-38, 1e-37)] +
                     [adversarial_vectors()[:21] * s for s in (1e-34, 1e-33)])


def f32_large():
    """(d) magnitudes up to the largest for which nothing in the reference's float statements overflows (TINY_LIMIT); the
    last scale lies beyond it on purpose: the rule has to reject it."""
    return np.vstack([_pixel_base() * s for s in (1e30, 1e33, 3e34, 1e35)])


def near_tie_detail_vectors(base, det_rows, det):
    """A strong base row r0 (step 0 takes it and unlocks its detail block) over an equal-weight sum of adjacent detail rows of
    that block and the base row next to r0: from step 1 on the tie is between rows of the unlocked block (kept in the
    Gram-updated pair scratch) and a base row (an MFMA row).  det: one channel's detail rows, blocks in base-row order."""
    off = np.concatenate([[0], np.cumsum(det_rows)])
    rng = np.random.default_rng(321)
    v = []
    for rep in range(48):
        r0 = int(rng.integers(1, 500))
        a = int(rng.integers(0, det_rows[r0] - 4))
        rows = [det[off[r0] + a + i] for i in range(2 + rep % 3)]
        v.append(base[r0] * 900.0 + (sum(rows) + base[r0 + 1]) * 300.0)
    return np.array(v)


def zero_and_sign_vectors(base):
    """The float flavour's `best_abs = -1` start (Eigen's maxCoeff): an all-zero vector selects row 0 with coefficient 0.
    All zeros, all negative zeros, and vectors whose projection on row 0 is exactly zero by construction (two elements
    v_j = c * row0_k, v_k = -c * row0_j with c a power of two: the two products are equal and cancel), both signs."""
    row0 = base[0].astype(np.float32).astype(np.float64)
    v = [np.zeros(64), -np.zeros(64)]
    for (j, k) in ((0, 1), (5, 58), (62, 63)):
        for c in (64.0, -64.0, 2.0 ** -10, 1024.0):
            e = np.zeros(64)
            e[j], e[k] = c * row0[k], -c * row0[j]
            v.append(e)
    for c in (1.0, -1.0):
        e = -np.zeros(64)
        e[9] = c * 2.0 ** -140                     # one subnormal element among negative zeros
        v.append(e)
    return np.array(v)


def vector_classes(base, det_rows, det_y):
    """name -> float64 [n, 64], every value as the builder made it (before the cast to f32 and before the rule)."""
    return {
        "adversarial": adversarial_vectors(),
        "near_ties_base": near_tie_vectors(base),
        "near_ties_detail": near_tie_detail_vectors(base, det_rows, det_y),
        "nan": nan_vectors(),
        "f32_subnormal_inputs": f32_subnormal_inputs(base),
        "f32_subnormal_products": f32_subnormal_products(),
        "f32_subnormal_residuals": f32_subnormal_residuals(),
        "f32_large": f32_large(),
        "zero_and_sign": zero_and_sign_vectors(base),
    }


# f32_large lies beyond the "table" rule by construction (it exists for the overflow edge of the tiny form)
FORMS_OF = {"f32_large": ("tiny",)}


def forms_of(name):
    return FORMS_OF.get(name, FORMS)


def as_f32(v):
    """CalcMPDynamicFast takes an Eigen::VectorXf: the float flavour's input is the f32 value, handed on as a double."""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def tiny_quant(v, K):
    """The step of the "tiny" form for one (f32-valued) vector: K equal steps."""
    m = float(np.nanmax(np.abs(v))) if np.isfinite(v).any() else 0.0
    return np.full(K, max(m * 2.0 ** -20, F32_MIN_NORMAL))


def well_defined(name, vectors, form):
    """The float flavour's rule (module docstring) on one class -> (kept [n, 64] as f32 values, rejected list of
    (index in `vectors`, reason))."""
    v32 = as_f32(vectors)
    keep, rejected = [], []
    limit, cmp = (TABLE_LIMIT, "<") if form == "table" else (TINY_LIMIT, "<=")
    for i in range(v32.shape[0]):
        x = v32[i]
        if name == "nan" and np.isnan(x).any():
            if np.isinf(x).any():
                rejected.append((i, "infinite as f32"))
            else:
                keep.append(i)
            continue
        if not np.isfinite(x).all():
            rejected.append((i, "not finite as f32"))
            continue
        m = np.abs(x).max()
        if (m < limit) if form == "table" else (m <= limit):
            keep.append(i)
        else:
            rejected.append((i, f"max|v| = {m:.3g}, the {form} form needs {cmp} {limit:g}"))
    return v32[keep], rejected


def float_cases(base, det_rows, det_y):
    """Every (class, form) of the float flavour after the rule: (name, form) -> (kept, rejected)."""
    out = {}
    for name, v in vector_classes(base, det_rows, det_y).items():
        for form in forms_of(name):
            out[(name, form)] = well_defined(name, v, form)
    return out


def f32_energy(res):
    """sum of squares as mpo_encode_tiles_fast forms it (float, element order, product and sum rounded separately); inf/nan
    where that sum overflows."""
    e = np.float32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        for x in np.asarray(res, np.float32):
            e = np.float32(e + np.float32(x * x))
    return float(e)


# ---- frames: a quantiser table that tells the flavours apart -----------------------------------------------------------

def fine_table(K):
    """With the context's own tables the float and the double oracle give the SAME container for most small frames (they differ in
    about 1 % of the tile-channels of a 1080p frame), so a frame test with those tables alone would pass a float context that ran
    the double kernel.  With every step 2^-12 the two differ in every tile row of the test frames (test_pursuit_cases.py).
    Well defined: pixel data give |v| <= 255 * 1.5, |best| <= 8 |v| < 2^12, |best / q| < 2^24.  (The container's header holds the
    table as u16, i.e. zeros: such a container is compared as bytes, not decoded.)"""
    return np.full((3, K), 2.0 ** -12)


# ---- the frame fuzzer's cases (tools/fuzz_parity.py, tests/test_gpu_fuzz_slice.py) --------------------------------------

def fuzz_frames(rng, cases, synth_frame):
    """Yields (W, H, K, bpp, kind, rgb): random small frames (at most 199 x 159), every K class, every quality, five kinds of
    content.  rng: a seed or a numpy Generator (a caller that passes a Generator may draw from it between two cases: the
    generator is lazy).  synth_frame(W, H, seed): the oracle's synthetic frame."""
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(rng)
    for n in range(cases):
        K = int(rng.choice([1, 2, 5, 8, 13, 16, 24, 32]))
        bpp = float(rng.choice([0.0, 0.5, 1.0, 2.0, 3.5, 5.0, 8.0]))
        W, H = int(rng.integers(1, 200)), int(rng.integers(1, 160))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif kind == 1:
            rgb = np.full((H, W, 3), rng.integers(0, 256, 3), dtype=np.uint8)
        elif kind == 2:
            rgb = synth_frame(W, H, int(rng.integers(0, 1 << 30)))
        elif kind == 3:                                            # smooth gradients with a few edges
            y, x = np.mgrid[0:H, 0:W]
            rgb = np.stack([(x * 3 + y) % 256, (x // 8 * 40) % 256, (y * 5) % 256], -1).astype(np.uint8)
        else:                                                     # sparse specks on black
            rgb = np.zeros((H, W, 3), np.uint8)
            m = rng.random((H, W)) < 0.02
            rgb[m] = rng.integers(0, 256, (int(m.sum()), 3), dtype=np.uint8)
        yield W, H, K, bpp, kind, rgb
