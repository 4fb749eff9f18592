"""The change tolerance on the host (no GPU): mpc_changed_tiles_tolerance is the numpy model of tests/tolerance_cases.py on every case,
at tolerance 0 it is mpc_changed_tiles, every wrong variant of the model differs from the model on some case, and every sequence the
device tests run has held, changed and byte-identical tiles, so that none of them can pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import delta_cases as dc
import tolerance_cases as tc


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


_CASES = {}


def cases(name, kind):
    if (name, kind) not in _CASES:
        _CASES[(name, kind)] = tc.tile_cases(name, kind)
    return _CASES[(name, kind)]


_MODEL = {}


def model(name, kind, k):
    """the model's answer to case k, computed once and shared"""
    if (name, kind, k) not in _MODEL:
        _, a, b, T = cases(name, kind)[k]
        _MODEL[(name, kind, k)] = tc.diff(a, b, T)
    return _MODEL[(name, kind, k)]


@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_the_host_definition_is_the_model(ia, name):
    n = 0
    for kind in tc.STRIDES:
        for k, (label, a, b, T) in enumerate(cases(name, kind)):
            want_list, want_sse, want_comp = model(name, kind, k)
            got_list, got_sse, got_comp = ia.changed_tiles_tolerance(a.pixels, b.pixels, T)
            assert got_list.dtype == np.int32 and got_sse.dtype == np.uint32
            assert np.array_equal(got_list, want_list), (name, label)
            assert np.array_equal(got_sse, want_sse), (name, label)
            assert np.array_equal(got_comp, want_comp), (name, label)
            assert int(want_sse.max()) <= tc.MAX_SSE
            n += 1
    assert n == 3 * 16


@pytest.mark.parametrize("name", list(tc.SHAPES))
def test_tolerance_0_is_changed_tiles(ia, name):
    for kind in tc.STRIDES:
        for label, a, b, _ in cases(name, kind):
            got = ia.changed_tiles_tolerance(a.pixels, b.pixels, 0)
            assert np.array_equal(got[0], ia.changed_tiles(a.pixels, b.pixels)), (name, label)
            assert np.array_equal(got[0], dc.changed_tiles(a.pixels, b.pixels)), (name, label)
            assert np.array_equal(got[2], b.pixels), (name, label)      # every tile that differs is taken: the composite is the frame


def test_the_cases_hold_what_they_promise():
    """the boundaries by name: exactly T held and T + 1 changed, 12 484 800 without overflow, a changed tile among held neighbours"""
    for name in tc.SHAPES:
        tx, ty = tc.grid(name)
        by_label = {label.split(" ", 1)[1]: (a, b, T) for label, a, b, T in cases(name, "tight")}
        seen = set()
        for flip in (0, 1):
            a, b, T = by_label[f"exact {flip}"]
            lst, sse, _ = tc.diff(a, b, T)
            marked = np.array(tc.marks(name))
            assert set(sse[marked].tolist()) <= {T, T + 1} and set(lst.tolist()) == set(marked[sse[marked] == T + 1].tolist())
            seen |= set(sse[marked].tolist())
        assert seen == {50, 51}
        a, b, T = by_label["0 to 255 below"]
        lst, sse, _ = tc.diff(a, b, T)
        assert sse.max() == tc.MAX_SSE == T + 1 or name == "tiny"
        assert len(lst) == (tc.SHAPES[name][0] // 8) * (tc.SHAPES[name][1] // 8)      # the whole tiles; a ragged one has fewer bytes
        a, b, T = by_label["0 to 255 at"]
        assert len(tc.diff(a, b, T)[0]) == 0
        a, b, T = by_label["T max"]
        lst, sse, comp = tc.diff(a, b, T)
        assert len(lst) == 0 and (sse > 0).all() and np.array_equal(comp, a.pixels)
        a, b, T = by_label["spread"]
        assert len(tc.diff(a, b, T)[0]) == (tx * ty + 1) // 2
        a, b, T = by_label["cross"]
        lst, sse, _ = tc.diff(a, b, T)
        flags = np.zeros((tx, ty), bool)
        flags.reshape(-1)[lst] = True
        for cx, cy in zip(*np.nonzero(flags)):
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= cx + dx < tx and 0 <= cy + dy < ty:
                    assert sse[(cx + dx) * ty + cy + dy] == T
        assert len(lst) >= 1
    # the shapes cross the seams they are there for
    assert tc.grid("ragged2") == (67, 4) and tc.SHAPES["ragged2"][1] % 8 == 5 and (3 * tc.SHAPES["ragged2"][0]) % 2 == 1
    assert tc.grid("word2")[0] == 66 and (3 * tc.SHAPES["word2"][0]) % 8 == 0
    assert tc.grid("blocks") == (130, 9) and 130 * 9 > 1024 and 130 > 128


@pytest.mark.parametrize("mistake", tc.WRONG)
def test_every_wrong_variant_is_told_from_the_model(mistake):
    caught = []
    for name in tc.SHAPES:
        for kind in tc.STRIDES:
            for k, (label, a, b, T) in enumerate(cases(name, kind)):
                want, got = model(name, kind, k), tc.diff(a, b, T, mistake)
                if not all(np.array_equal(x, y) for x, y in zip(want, got)):
                    caught.append((name, label))
    assert caught, mistake
    if mistake == "kept copy updated for held tiles":                   # compares with the previous frame: the ramp never fires
        frames, T, name = tc.sequence("ramp word2")
        assert all(len(r["list"]) == 0 for r in tc.replay(frames, T, mistake)[1:])
        assert any(len(r["list"]) == 1 for r in tc.replay(frames, T)[1:])


@pytest.mark.parametrize("label", list(tc.SEQUENCES))
def test_every_sequence_holds_changes_and_repeats(ia, label):
    frames, T, name = tc.sequence(label)
    assert len(frames) >= 6
    calls = tc.replay(frames, T)
    held = changed = same = 0
    for i, r in enumerate(calls[1:], 1):
        held += r["held"]
        changed += len(r["list"])
        same += int((r["sse"] == 0).sum())
        assert r["held"] == int(((r["sse"] > 0) & (r["sse"] <= T)).sum())
        # every tile of the composite is within the tolerance of the frame's
        assert dc.changed_tiles(r["composite"], frames[i]).size == r["held"]
        assert (tc.diff_pixels(r["composite"], frames[i], T)[1] <= T).all()
        # and the host definition walks the same way
        got = ia.changed_tiles_tolerance(calls[i - 1]["composite"], frames[i], T)
        assert np.array_equal(got[0], r["list"]) and np.array_equal(got[1], r["sse"]) and np.array_equal(got[2], r["composite"])
    assert held > 0 and changed > 0 and same > 0, (label, held, changed, same)
    assert all(len(r["list"]) < len(calls[0]["list"]) for r in calls[1:])


def test_the_ramp_fires_when_its_sum_first_exceeds_the_tolerance():
    for label in ("ramp word2", "ramp ragged2"):
        frames, T, name = tc.sequence(label)
        tile = tc.ramp_sequence(name)[2]
        calls = tc.replay(frames, T)
        fired = [i for i, r in enumerate(calls) if i and len(r["list"])]
        assert fired == [3, 6] and all(calls[i]["list"].tolist() == [tile] for i in fired)      # 192 j^2 > 1000 first at j = 3, then again from there
        assert [int(r["sse"][tile]) for r in calls[1:]] == [192, 768, 1728, 192, 768, 1728, 192]


def test_refusals(ia):
    L = ia.load_library()
    a = np.zeros((8, 8, 3), np.uint8)
    tiles, n, sse = np.zeros(1, np.int32), C.c_int(-1), np.zeros(1, np.uint32)
    p, s = tiles.ctypes.data_as(C.POINTER(C.c_int32)), sse.ctypes.data_as(C.POINTER(C.c_uint32))
    A = ia.api.MPC_ERR_ARGUMENT
    assert L.mpc_changed_tiles_tolerance(None, 0, a.ctypes.data, 0, 8, 8, 8, 5, p, C.byref(n), s) == A
    assert L.mpc_changed_tiles_tolerance(a.ctypes.data, 0, None, 0, 8, 8, 8, 5, p, C.byref(n), s) == A
    assert L.mpc_changed_tiles_tolerance(a.ctypes.data, 0, a.ctypes.data, 0, 8, 8, 8, 5, None, C.byref(n), s) == A
    assert L.mpc_changed_tiles_tolerance(a.ctypes.data, 0, a.ctypes.data, 0, 8, 8, 8, 5, p, None, s) == A
    for w, h, bs, stride in ((0, 8, 8, 0), (8, 0, 8, 0), (8, 8, 0, 0), (8, 8, 9, 0), (8, 8, 8, 23)):
        assert L.mpc_changed_tiles_tolerance(a.ctypes.data, stride, a.ctypes.data, 0, w, h, bs, 5, p, C.byref(n), s) == A
    assert n.value == -1
    assert L.mpc_changed_tiles_tolerance(a.ctypes.data, 0, a.ctypes.data, 0, 8, 8, 8, 5, p, C.byref(n), None) == ia.api.MPC_OK and n.value == 0
    assert L.mpc_delta_set_tolerance(None, 5) == A and L.mpc_delta_tolerance(None) == 0
    assert L.mpc_delta_held(None, None, None) == A and L.mpc_delta_frame(None, None, 0) == A and L.mpc_delta_frame_device(None, None) == A
