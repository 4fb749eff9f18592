"""Oracle (plain C) vs the REFERENCE's own object code (oracle/_ref/libref.so =
SimpleMatrix + ImageHelper/misc compiled in place from the reference tree).
Everything here must agree bit-for-bit.

What libref.so computes on every input below is kept in tests/golden/ref_vectors.npz (outputs, keyed by case, with a
digest of the inputs they were computed from), so the oracle is checked against the reference's results wherever the
suite runs; where libref.so has been built, its live results are checked as well.  To rewrite the file from libref.so:

    MPC_RECORD_REF_VECTORS=1 python -m pytest tests/test_oracle_ref.py
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN

VECTORS = os.path.join(GOLDEN, "ref_vectors.npz")


def _digest(inputs):
    h = hashlib.sha256()
    for x in inputs:
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def _live_ops(oracle, R):
    """libref.so's entry points on numpy arrays."""
    def symm_eigen(A):
        n = A.shape[0]
        v, e = np.zeros((n, n)), np.zeros(n)
        R.ref_symm_eigen(oracle._dp(A), n, oracle._dp(v), oracle._dp(e))
        return v, e

    def multiply(D, X):                                   # one math::Multiply(Matrix, Vector) per row of X
        P = np.zeros((X.shape[0], D.shape[0]))
        for j in range(X.shape[0]):
            p = np.zeros(D.shape[0])
            R.ref_multiply(oracle._dp(D), D.shape[0], D.shape[1], oracle._dp(np.ascontiguousarray(X[j])), oracle._dp(p))
            P[j] = p
        return (P,)

    def scale_subtract(r, atom, coeff):
        rr = r.copy()
        R.ref_scale_subtract(oracle._dp(rr), oracle._dp(atom), float(coeff[0]), r.shape[0])
        return (rr,)

    def yuv_from_rgb(cols):
        out = np.zeros((cols.shape[0], 3))
        y = np.zeros(3)
        for i, (r8, g8, b8) in enumerate(cols.tolist()):
            R.ref_yuv_from_rgb(r8, g8, b8, oracle._dp(y))
            out[i] = y
        return (out,)

    def rgb_from_yuv(yuv):
        out = np.zeros((yuv.shape[0], 3), np.uint8)
        o = np.zeros(3, np.uint8)
        for i, (yy, uu, vv) in enumerate(yuv.tolist()):
            R.ref_rgb_from_yuv(yy, uu, vv, o.ctypes.data_as(C.POINTER(C.c_uint8)))
            out[i] = o
        return (out,)

    return {"symm_eigen": symm_eigen, "multiply": multiply, "scale_subtract": scale_subtract, "yuv_from_rgb": yuv_from_rgb,
            "rgb_from_yuv": rgb_from_yuv}


class Reference:
    """ref(op, key, *inputs) -> the reference's outputs: computed by libref.so (live; optionally recorded into `record`)
    or read from the stored vectors, which must have been computed from the same inputs."""

    def __init__(self, ops=None, stored=None, record=None):
        self.ops, self.stored, self.record = ops, stored, record

    def __call__(self, op, key, *inputs):
        key = f"{op}/{key}"
        if self.ops is None:
            assert str(self.stored[key + "/in"]) == _digest(inputs), f"{key}: inputs differ from the recorded ones"
            return tuple(self.stored[f"{key}/{i}"] for i in range(int(self.stored[key + "/n"])))
        out = self.ops[op](*inputs)
        if self.record is not None:
            self.record[key + "/in"] = np.array(_digest(inputs))
            self.record[key + "/n"] = np.array(len(out))
            for i, o in enumerate(out):
                self.record[f"{key}/{i}"] = o
        return out


@pytest.fixture(scope="module")
def refs(oracle):
    """the stored vectors, and libref.so itself where it has been built"""
    live = oracle.ref()
    if os.environ.get("MPC_RECORD_REF_VECTORS"):
        assert live is not None, "recording needs oracle/_ref/libref.so"
        record = {}
        yield [Reference(ops=_live_ops(oracle, live), record=record)]
        np.savez_compressed(VECTORS, **record)
        return
    with np.load(VECTORS) as z:
        stored = dict(z)
    yield [Reference(stored=stored)] + ([Reference(ops=_live_ops(oracle, live))] if live is not None else [])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13, 31, 32, 47, 63, 64])
def test_symmetric_eigensolver_bit_exact(oracle, refs, n):
    """symmeigen.cpp:34-244 vs mpo_symm_eigen on model covariances and random symmetric input."""
    L = oracle.lib()
    rng = np.random.default_rng(n)
    pts = [(x, y) for x in range(8) for y in range(8)][:n]
    cases = []
    for ch in range(3):
        cases.append(np.array([[L.mpo_cov_model(ch, float(a[0] - b[0]), float(a[1] - b[1])) for b in pts]
                               for a in pts]))
    m = rng.standard_normal((n, n))
    cases.append(m + m.T)
    cases.append(np.diag(rng.standard_normal(n)))        # already diagonal: scale == 0 branch
    for c, A in enumerate(cases):
        A = np.ascontiguousarray(A)
        v1, e1 = np.zeros((n, n)), np.zeros(n)
        L.mpo_symm_eigen(oracle._dp(A), n, oracle._dp(v1), oracle._dp(e1))
        for ref in refs:
            v2, e2 = ref("symm_eigen", f"{n}/{c}", A)
            assert (_bits(v1) == _bits(v2)).all()
            assert (_bits(e1) == _bits(e2)).all()


def test_gemv_row_order_bit_exact(oracle, refs, octx32):
    """math::Multiply(Matrix,Vector) mathmatrix.cpp:426 == sequential tot += l*r (the oracle's row_dot),
    checked through mpo_calc_mp's first selection on real dictionary rows."""
    rng = np.random.default_rng(7)
    D = np.ascontiguousarray(np.vstack([octx32.base, octx32.det[0][:63]]))
    X = np.stack([rng.standard_normal(64) * rng.choice([1.0, 30.0, 500.0]) for _ in range(20)])
    for ref in refs:
        (P,) = ref("multiply", "dictionary_rows", D, X)
        for r, p in zip(X, P):
            r = np.ascontiguousarray(r)
            # reference Select (MatchingPursuit.cpp:7-25) on the reference's projections
            best, idx = 0.0, -1
            for i in range(510):
                if abs(p[i]) > abs(best):
                    best, idx = p[i], i
            cnt, d, k, res, S = octx32.calc_mp(0, r, quant=np.ones(32))
            assert d[0] == idx
            q = int(np.sign(best) * np.floor(abs(best) + 0.5))            # round half away, quant = 1
            assert k[0] == ((q << 1) ^ (q >> 31)) & 0xFFFF


def test_scale_subtract_bit_exact(oracle, refs, octx32):
    """residual update MatchingPursuit.cpp:70-71 via Vector::Scale/Subtract: one full MP step."""
    rng = np.random.default_rng(11)
    for j in range(20):
        r = np.ascontiguousarray(rng.standard_normal(64) * 200.0)
        q = np.full(32, 1.0e9)
        q[0] = 3.0                                   # step 1 quantises to 0 -> count == 1, residual after 1 update
        cnt, d, k, res, S = octx32.calc_mp(0, r, quant=q)
        if cnt != 1:
            continue
        coeff = 3.0 * float(oracle.lib().mpo_zigzag_dec(int(k[0])))
        for ref in refs:
            (rr,) = ref("scale_subtract", str(j), r, np.ascontiguousarray(octx32.base[d[0]]), np.array([coeff]))
            assert (_bits(rr) == _bits(res)).all()


def test_yuv_rgb_bit_exact(oracle, refs):
    """img::YUVFromRGB / RGBFromYUV misc.cpp:7-36."""
    L = oracle.lib()
    rng = np.random.default_rng(3)
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    cols = np.array(rng.integers(0, 256, (5000, 3)).tolist() + [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]],
                    np.uint8)
    yuvs = rng.standard_normal((5000, 3)) * [120, 80, 80] + [128, 0, 0]
    for ref in refs:
        (want,) = ref("yuv_from_rgb", "colours", cols)
        for (r8, g8, b8), y in zip(cols.tolist(), want):
            L.mpo_yuv_from_rgb(r8, g8, b8, C.byref(a), C.byref(b), C.byref(c))
            assert (a.value, b.value, c.value) == tuple(y)
        out1 = (C.c_uint8 * 3)()
        (want,) = ref("rgb_from_yuv", "colours", yuvs)
        for (yy, uu, vv), out2 in zip(yuvs.tolist(), want):
            L.mpo_rgb_from_yuv(yy, uu, vv, C.cast(C.byref(out1, 0), C.POINTER(C.c_uint8)),
                               C.cast(C.byref(out1, 1), C.POINTER(C.c_uint8)),
                               C.cast(C.byref(out1, 2), C.POINTER(C.c_uint8)))
            assert tuple(out1) == tuple(out2)
