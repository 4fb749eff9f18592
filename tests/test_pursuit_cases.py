"""The inputs of the pursuit parity tests (tests/pursuit_cases.py), checked on the CPU with both oracles: no class is dropped
silently by the well-definedness rule, every class does in the oracle what its name says, and the float cases can tell float
arithmetic from double arithmetic at all.  Every count is an exact expected value, so a change of a builder shows here.

Why this matters for the GPU tests: test_gpu_fast_parity.py asserts bit equality with OracleFastContext on these inputs.  With
the context's tables the float and the double oracle agree on EVERY kept case (EXPECTED[..., "table"]["separating"] == 0
throughout), so that form alone would not notice a float kernel that computed in double; the tiny-quant form separates the two
oracles on more than half of its cases."""
import numpy as np
import pytest

import pursuit_cases as pc

K = 32


def _subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < np.float32(pc.F32_MIN_NORMAL))


def _same(a, b):
    (c1, d1, k1, _, s1), (c2, d2, k2, _, s2) = a, b
    n = min(c1, K - 1) + 1
    return c1 == c2 and (d1[:n] == d2[:n]).all() and (k1[:n] == k2[:n]).all() and s1 == s2


def _quant_of(form, v):
    """the step table of a form for one vector: None (the context's) or the tiny step as the f32 value the float oracle uses"""
    if form == "table":
        return None
    return pc.tiny_quant(v, K).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def ofast32(oracle, octx32):
    return oracle.OracleFastContext(octx32)


@pytest.fixture(scope="module")
def cases(octx32):
    return pc.float_cases(octx32.base, octx32.det_rows, octx32.det[0])


@pytest.fixture(scope="module")
def stats(octx32, ofast32, cases):
    """per (class, form): what the two oracles do with the kept cases, channel 0"""
    base32 = octx32.base.astype(np.float32)
    out = {}
    for (name, form), (kept, rejected) in cases.items():
        s = dict(kept=len(kept), rejected=len(rejected), full=0, count0=0, separating=0, all_inputs_subnormal=0,
                 no_input_subnormal=0, subnormal_products=0, subnormal_residuals=0)
        for v in kept:
            q = _quant_of(form, v)
            if q is not None:
                assert np.float32(q[0]) >= np.float32(pc.F32_MIN_NORMAL) and np.isfinite(np.float32(q[0]))   # normal, non-zero f32
            f = ofast32.calc_mp(0, v, quant=q)
            d = octx32.calc_mp(0, v, quant=q)
            cnt, res = f[0], f[3]
            assert 0 <= cnt <= K
            if not np.isnan(v).any():
                assert np.isfinite(res).all(), (name, form)          # no float intermediate overflowed on the way
                assert np.isfinite(d[3]).all(), (name, form)
            s["full"] += cnt == K
            s["count0"] += cnt == 0
            s["separating"] += not _same(f, d)
            v32 = v.astype(np.float32)
            nz = v32 != 0
            s["all_inputs_subnormal"] += bool(nz.any() and _subnormal(v32)[nz].all())
            s["no_input_subnormal"] += not _subnormal(v32).any()
            with np.errstate(invalid="ignore"):
                s["subnormal_products"] += bool(_subnormal(base32 * v32[None, :]).any())
            s["subnormal_residuals"] += bool(_subnormal(res).any())
        out[(name, form)] = {k: int(x) for k, x in s.items()}
    return out


def _row(kept, rejected, full, count0, separating, all_sub, no_sub, sub_prod, sub_res):
    return dict(kept=kept, rejected=rejected, full=full, count0=count0, separating=separating, all_inputs_subnormal=all_sub,
                no_input_subnormal=no_sub, subnormal_products=sub_prod, subnormal_residuals=sub_res)


# kept, rejected by the rule, count == K, count == 0, float oracle != double oracle, vectors whose non-zero inputs are all f32
# subnormals, vectors without a subnormal input, vectors with a subnormal product against a base row at step 0, vectors whose
# final float residual holds a subnormal -- measured with oracle/mpo_fast.c and oracle/mpo_mp.c, channel 0, K = 32, quality 3.5
EXPECTED = {
    ("adversarial", "table"): _row(108, 36, 6, 79, 0, 6, 98, 12, 10),
    ("adversarial", "tiny"): _row(120, 24, 86, 19, 74, 6, 110, 12, 12),
    ("near_ties_base", "table"): _row(96, 0, 48, 0, 0, 0, 96, 0, 0),
    ("near_ties_base", "tiny"): _row(96, 0, 96, 0, 75, 0, 96, 0, 0),
    ("near_ties_detail", "table"): _row(48, 0, 3, 0, 0, 0, 48, 0, 0),
    ("near_ties_detail", "tiny"): _row(48, 0, 48, 0, 38, 0, 48, 0, 0),
    ("nan", "table"): _row(12, 0, 7, 5, 0, 0, 12, 0, 0),
    ("nan", "tiny"): _row(12, 0, 7, 5, 4, 0, 12, 0, 0),
    ("f32_subnormal_inputs", "table"): _row(36, 0, 0, 36, 0, 36, 0, 36, 36),
    ("f32_subnormal_inputs", "tiny"): _row(36, 0, 10, 12, 11, 36, 0, 36, 36),
    ("f32_subnormal_products", "table"): _row(24, 0, 0, 24, 0, 0, 24, 24, 0),
    ("f32_subnormal_products", "tiny"): _row(24, 0, 24, 0, 3, 0, 24, 24, 2),
    ("f32_subnormal_residuals", "table"): _row(66, 0, 0, 66, 0, 0, 66, 32, 0),
    ("f32_subnormal_residuals", "tiny"): _row(66, 0, 36, 0, 29, 0, 66, 32, 50),
    ("f32_large", "tiny"): _row(18, 6, 18, 0, 15, 0, 18, 0, 0),
    ("zero_and_sign", "table"): _row(16, 0, 0, 9, 0, 2, 14, 2, 2),
    ("zero_and_sign", "tiny"): _row(16, 0, 12, 4, 4, 2, 14, 2, 2),
}
# adversarial_vectors()' six pixel vectors per magnitude that run all K steps with the tiny step: float oracle (kept magnitudes),
# double oracle (the double test's magnitudes)
EXPECTED_FULL_FLOAT = {1e-300: 0, 1e-160: 0, 1e-45: 0, 1e-38: 6, 1e-30: 6, 1e-10: 6, 1.0: 6, 1e10: 6, 1e30: 6}
EXPECTED_FULL_DOUBLE = {1e-300: 0, 1e-160: 6, 1e-45: 6, 1e-38: 6, 1e-30: 6, 1e-10: 6, 1.0: 6, 1e10: 6, 1e30: 6, 1e38: 6, 1e39: 6}
EXPECTED_TINY_TOTAL = (436, 253)          # kept tiny-form cases, of which the two oracles differ: 58 %


def test_no_class_is_dropped_silently(cases):
    classes = {name for name, _ in cases}
    assert classes == {"adversarial", "near_ties_base", "near_ties_detail", "nan", "f32_subnormal_inputs",
                       "f32_subnormal_products", "f32_subnormal_residuals", "f32_large", "zero_and_sign"}
    for (name, form), (kept, rejected) in cases.items():
        total = len(kept) + len(rejected)
        assert len(kept) > 0, (name, form)
        assert 4 * len(rejected) <= total, (name, form, len(rejected), total)        # at most 25 % of a class
        assert all(reason for _, reason in rejected)
    for name in classes:                                                             # every class runs in the carrying form
        assert "tiny" in pc.forms_of(name)
    assert pc.forms_of("f32_large") == ("tiny",)                                     # beyond the table rule by construction


def test_the_rule_keeps_only_defined_cases(cases):
    for (name, form), (kept, _) in cases.items():
        assert (kept.astype(np.float32).astype(np.float64) == kept)[~np.isnan(kept)].all()      # f32 values
        assert not np.isinf(kept).any()
        clean = kept[~np.isnan(kept).any(axis=1)]
        assert name == "nan" or len(clean) == len(kept)
        m = np.abs(clean).max(axis=1)
        assert (m < pc.TABLE_LIMIT).all() if form == "table" else (m <= pc.TINY_LIMIT).all()
        # the bound that makes the float statements finite: 8 max|v| in f32
        assert np.isfinite((np.float32(8) * m.astype(np.float32))).all()


def test_every_class_does_what_its_name_says(stats):
    assert stats == EXPECTED
    for form in pc.FORMS:
        a = stats[("f32_subnormal_inputs", form)]
        assert a["all_inputs_subnormal"] == a["kept"]                       # (a) nothing but subnormals and zeros
        b = stats[("f32_subnormal_products", form)]
        assert b["no_input_subnormal"] == b["kept"] and b["subnormal_products"] == b["kept"]      # (b)
        c = stats[("f32_subnormal_residuals", form)]
        assert c["no_input_subnormal"] == c["kept"]                         # (c) subnormal only after some steps
    assert stats[("f32_subnormal_residuals", "tiny")]["subnormal_residuals"] >= 40
    assert stats[("f32_large", "tiny")]["full"] == stats[("f32_large", "tiny")]["kept"]
    assert stats[("near_ties_base", "tiny")]["full"] == 96 and stats[("near_ties_detail", "tiny")]["full"] == 48


def test_tiny_quant_form_separates_float_from_double(stats):
    """the condition: at least half of all kept tiny-form cases give different records in the two oracles, and every class has
    such a case, except those that cannot by construction (pc.CANNOT_SEPARATE: no arithmetic that could differ happens in a
    zero vector or before a NaN ends the pursuit)."""
    tiny = {name: s for (name, form), s in stats.items() if form == "tiny"}
    kept = sum(s["kept"] for s in tiny.values())
    separating = sum(s["separating"] for s in tiny.values())
    assert (kept, separating) == EXPECTED_TINY_TOTAL
    assert 2 * separating >= kept
    for name, s in tiny.items():
        if name not in pc.CANNOT_SEPARATE:
            assert s["separating"] >= 1, name
    assert set(pc.CANNOT_SEPARATE) == {"zero_and_sign", "nan"}
    # and the table form does not separate them at all: it guards the screen's thresholds, not the arithmetic
    assert sum(s["separating"] for (name, form), s in stats.items() if form == "table") == 0


def test_tiny_quant_reaches_all_steps_at_every_magnitude(octx32, ofast32):
    """adversarial_vectors() scales six pixel vectors by thirteen magnitudes (rows 25 .. 102): per magnitude, how many of
    the six run all K steps with the tiny step.  Float: the magnitudes that survive the rule; those whose step is clamped
    to 2^-126 (inputs that are zero or subnormal in f32) cannot run at all."""
    v = pc.adversarial_vectors()
    scales = (1e-300, 1e-160, 1e-45, 1e-38, 1e-30, 1e-10, 1.0, 1e10, 1e30, 1e38, 1e39, 1e150, 1e300)
    full_f, full_d = {}, {}
    for n, s in enumerate(scales):
        block = v[25 + 6 * n: 31 + 6 * n]
        assert 200 * s < np.abs(block).max() <= 255 * s * (1 + 1e-12)
        kept, _ = pc.well_defined("adversarial", block, "tiny")
        if len(kept):
            full_f[s] = sum(ofast32.calc_mp(0, x, quant=_quant_of("tiny", x))[0] == K for x in kept)
        if s < 1e100:                                                        # the double test's own rule
            full_d[s] = sum(octx32.calc_mp(0, x, quant=np.full(K, max(np.abs(x).max(), 1e-290) * 2.0 ** -20))[0] == K for x in block)
    assert full_f == EXPECTED_FULL_FLOAT
    assert full_d == EXPECTED_FULL_DOUBLE
    for s, n in full_f.items():
        if 255 * s * 2.0 ** -20 >= pc.F32_MIN_NORMAL:
            assert n >= 1, s
    for s, n in full_d.items():
        if s >= 1e-290:
            assert n >= 1, s


def test_zero_vector_semantics_of_the_two_flavours(octx32, ofast32):
    """float: maxCoeff's first maximum of an all-zero |p| is row 0 with coefficient 0 -> count 0, record (0, 0), 510 rows swept;
    double: nothing compares greater than 0, index -1 -> the same outputs by the other path (MatchingPursuit.cpp:50-54).
    A vector orthogonal to row 0 must not end there: row 0 is only the first candidate."""
    z = pc.zero_and_sign_vectors(octx32.base)
    for v in z[:2]:
        for o in (ofast32, octx32):
            cnt, d, k, res, S = o.calc_mp(0, v)
            assert (cnt, int(d[0]), int(k[0]), S) == (0, 0, 0, 510)
            assert not res.any()
    row0 = octx32.base[0].astype(np.float32)
    for v in pc.as_f32(z[2:14]):
        p0 = np.float32(0)
        for j in range(64):
            p0 = np.float32(p0 + np.float32(row0[j] * np.float32(v[j])))
        assert p0 == 0                                                       # orthogonal to row 0 in float, exactly
        cnt, d, k, res, S = ofast32.calc_mp(0, v, quant=_quant_of("tiny", v))
        assert cnt > 0 and d[0] != 0


def test_double_cases_are_kept_as_the_double_tests_filter_them(octx32):
    """test_gpu_parity.py's own filters on the moved builders: nothing lost by the move"""
    v = pc.adversarial_vectors()
    assert v.shape == (144, 64)
    assert (np.abs(v).max(axis=1) < 1e6).sum() == 108 and (np.abs(v).max(axis=1) < 1e100).sum() == 132
    assert pc.near_tie_vectors(octx32.base).shape == (96, 64)
    n = pc.nan_vectors()
    assert n.shape == (12, 64) and np.isnan(n).any(axis=1).sum() == pc.NAN_ROWS and np.isnan(n[:pc.NAN_ROWS]).any(axis=1).all()
    for i, x in enumerate(n):
        assert (octx32.calc_mp(0, x)[0] == 0) == (i < pc.NAN_ROWS)
    for x in v[np.abs(v).max(axis=1) < 1e6]:
        cnt, d, k, res, S = octx32.calc_mp(0, x)
        assert np.isfinite(res).all()
    frames = pc.degenerate_frames(8)
    assert list(frames) == ["black", "white", "grey", "checker", "stripes", "hard noise", "one pixel", "one column"]


@pytest.mark.parametrize("K,size,seed", [(16, (328, 208), 77), (8, (136, 100), 40), (32, (200, 136), 4000), (8, (97, 83), 4000)])
def test_fine_table_separates_the_flavours_in_every_tile_row(oracle, K, size, seed):
    """the frames of the workgroup-limit, batch-stripe and multi-lane tests: with pc.fine_table every tile row holds a
    tile whose records differ between the float and the double oracle, so every stripe of those tests shows its flavour"""
    o = oracle.OracleContext(K, 8, 3.5)
    f = oracle.OracleFastContext(o)
    rgb = oracle.synth_frame(size[0], size[1], seed)
    q = pc.fine_table(K)
    a, b = o.encode_tiles(rgb, quant=q), f.encode_tiles(rgb, quant=q)
    tiles_y = (size[1] + 7) // 8
    differ = (a[0] != b[0]).any(axis=1) | (a[1] != b[1]).any(axis=(1, 2)) | (a[2] != b[2]).any(axis=(1, 2))
    assert set(np.nonzero(differ)[0] % tiles_y) == set(range(tiles_y))
    assert o.encode_image(rgb, quant=q) != f.encode_image(rgb, quant=q)


def test_fuzz_generator_is_reproducible(oracle):
    a = list(pc.fuzz_frames(20241016, 6, oracle.synth_frame))
    b = list(pc.fuzz_frames(np.random.default_rng(20241016), 6, oracle.synth_frame))
    assert [x[:5] for x in a] == [x[:5] for x in b]
    assert all((x[5] == y[5]).all() for x, y in zip(a, b))
    assert all(x[5].shape == (x[1], x[0], 3) and x[0] < 200 and x[1] < 160 for x in a)
