"""The frames of trip_cases on the host (no GPU): they hold what they are for, every host definition gives their numpy expectation,
the oracle writes the same container, the numpy model of the block loops gives the expectation, and each wrong variant of that
model changes a named smallest case.  Every equality is exact."""
import numpy as np
import pytest

import trip_cases as tc


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def test_the_frames_cover_what_they_are_meant_to(ia):
    tc.check_coverage(ia)


def test_numpy_run_lengths_are_the_hosts(ia):
    for name in tc.FRAMES:
        for s in tc.frame(name)["as_coded"]:
            assert np.array_equal(tc.rle_encode(s), ia.run_length_encode(s))
            assert np.array_equal(tc.expand(tc.rle_encode(s), 0, len(tc.rle_encode(s)), 0, 0)[0], s)
    for held in tc.plan_cases().values():
        assert np.array_equal(tc.rle_encode(held), ia.run_length_encode(held))


@pytest.mark.parametrize("name", tc.FRAMES)
def test_oracle_writes_the_same_container(ia, oracle, name):
    f = tc.frame(name)
    want = oracle.write_compressed(dict(W=f["W"], H=f["H"], K=f["K"], bs=8, quant=f["quant"], lengths=f["counts"], codes=f["as_held"]))
    assert bytes(want) == tc.container(name)


@pytest.mark.parametrize("name", tc.FRAMES)
def test_serial_parses_give_the_expectation(ia, name):
    f = tc.frame(name)
    s = ia.read_compressed(tc.container(name))
    assert np.array_equal(s["lengths"], f["counts"])
    for i, (got, want) in enumerate(zip(s["codes"], f["want"])):
        assert np.array_equal(got, want), i
    lossy = [i for i in range(6 * f["K"]) if not np.array_equal(f["want"][i], f["as_held"][i])]
    assert lossy == [1, 2 * f["K"] + 1, 4 * f["K"] + 1]             # every walk holds steps the 16-bit differences cannot
    for interval in tc.INTERVALS:
        for index in (ia.container_index(tc.container(name), interval), tc.index(name, interval)):
            got, route = ia.parse_container_by_index(tc.container(name), index)
            assert route == 0 and np.array_equal(got, tc.expected_serial(name)), interval


@pytest.mark.parametrize("rect_name", tc.RECTS)
def test_host_window_gives_the_expectation(ia, rect_name):
    name, rect, _ = tc.RECTS[rect_name]
    want, want_ranges = tc.expected_window(name, rect)
    sizes = tc.window_sizes(name, want_ranges)
    for interval in tc.INTERVALS:
        for parse_all in (False, True):
            got, ranges, route = ia.parse_container_window_by_index(tc.container(name), tc.index(name, interval), rect, parse_all)
            assert route == 0 and np.array_equal(ranges, want_ranges), (interval, parse_all)
            assert tc.first_difference(got, want, sizes, True) is None, (interval, parse_all)


@pytest.mark.parametrize("name", tc.FRAMES)
def test_numpy_aux_entries_are_the_hosts(ia, name):
    f = tc.frame(name)
    coded, packed = tc.packed_form(name)
    for interval in tc.INTERVALS:
        for i in range(6 * f["K"]):
            got = ia.index_aux(tc.index(name, interval), i + 1)
            dc = tc.is_dc(i, f["K"])
            if not (packed[i] or dc):
                assert len(got["out"]) == 0
                continue
            at = np.arange(0, len(coded[i]), interval)
            for key, arr in zip(("out", "prev", "state", "dc"), tc.aux_arrays(coded[i], packed[i], dc)):
                assert np.array_equal(got[key], arr[at]), (interval, i, key)


# ---- the model of the loops ----
@pytest.mark.parametrize("name", tc.FRAMES)
def test_model_of_the_whole_unpack_gives_the_expectation(ia, name):
    f = tc.frame(name)
    for force in (False, True):
        coded, packed = tc.coded_form(f["as_coded"], force)
        for i, (c, p) in enumerate(zip(coded, packed)):
            if not p:
                continue
            got = tc.window_model(c, tc.whole(c, len(f["as_coded"][i])))
            assert got is not None and np.array_equal(got, f["as_coded"][i]), (force, i)
            if tc.is_dc(i, f["K"]):
                w = dict(out0=0, out1=len(got), dc0=0)
                assert np.array_equal(tc.dc_model(got, w), f["want"][i]), i
                assert (len(got) > tc.DC_THREADS * tc.UNPACK_BLOCK) == (not np.array_equal(tc.dc_model(got, w, "dc_carry_256"), f["want"][i]))
            if len(c) > tc.TRIP * tc.UNPACK_BLOCK and not force:
                # every packed stream of more than 64 blocks shows a lost `run`; a lost `state` only where the trip cuts a pair or
                # stands in front of a count, which is what the barely packed streams 0 and 8 are built for
                assert tc.window_model(c, tc.whole(c, len(f["as_coded"][i])), "run_lost") is None, i
                if i in (0, 8):
                    assert tc.window_model(c, tc.whole(c, len(f["as_coded"][i])), "state_lost") is None, i
        assert tc.plan_model(f["as_coded"][0]) == len(tc.rle_encode(f["as_coded"][0]))
    # B's stream 0 is the one a plan that loses run_before at block 64 gets wrong, and it comes out shorter
    b = tc.frame("B")["as_coded"]
    assert [tc.plan_model(s, "run_before_lost") - tc.plan_model(s) for s in b] == [-1, 0, 0, 0, 0, 0]
    assert all(tc.plan_model(s) == len(tc.rle_encode(s)) for s in b)


@pytest.mark.parametrize("rect_name", ["A_far", "A_span", "B_span", "B_mid", "B_last", "B_dc"])
def test_model_of_the_window_gives_the_expectation(ia, rect_name):
    name, rect, _ = tc.RECTS[rect_name]
    f = tc.frame(name)
    coded, _ = tc.packed_form(name)
    interval = 100
    two_trips = 0
    for w in tc.windows(ia, name, rect, interval):
        i = w["i"]
        mem = coded[i].copy()
        mem[:w["s0"]] = 0xA5A5                                       # not parsed
        mem[w["s1"]:] = 0xA5A5
        got = tc.window_model(mem, w) if w["packed"] else mem[w["out0"]:w["out1"]]
        assert got is not None, i
        if w["dc"]:
            z = np.zeros(w["expect"], np.uint16)
            z[w["out0"]:w["out1"]] = got
            got = tc.dc_model(z, w)
            if w["out0"] // tc.UNPACK_BLOCK + tc.DC_THREADS < w["out1"] // tc.UNPACK_BLOCK:
                assert not np.array_equal(tc.dc_model(z, w, "dc_carry_256"), got), i
        assert np.array_equal(got, f["want"][i][w["out0"]:w["out1"]]), i
        if w["packed"] and w["k1"] - w["k0"] > tc.TRIP:
            two_trips += 1
            assert tc.window_model(mem, w, "run_lost") is None, i
    assert two_trips >= (3 if rect_name in ("B_span", "B_dc") else 0)
    if rect_name == "B_span":                                       # stream 0 has a pair and a count across the window's own trips
        w = [w for w in tc.windows(ia, name, rect, interval) if w["i"] == 0][0]
        assert w["k0"] == 31 and tc.window_model(coded[0], w, "state_lost") is None


# ---- each wrong variant changes a named smallest case ----
def _same(got, want):
    return got is not None and np.array_equal(got, want)


@pytest.mark.parametrize("case", list(tc.window_cases()))
def test_right_window_model_on_the_small_cases(case):
    c = tc.window_cases()[case]
    assert _same(tc.window_model(c["mem"], c["w"]), c["want"])


@pytest.mark.parametrize("variant", [v for v in tc.WINDOW_VARIANTS if v != "exit_unchecked"])
def test_every_window_variant_changes_its_smallest_case(variant):
    cases = tc.window_cases()
    c = cases[tc.WINDOW_SMALLEST[variant]]
    assert not _same(tc.window_model(c["mem"], c["w"], variant), c["want"])
    for smaller in tc.WINDOW_SMALLER[variant]:
        s = cases[smaller]
        assert _same(tc.window_model(s["mem"], s["w"], variant), s["want"]), smaller


def test_more_of_the_window_variants():
    cases = tc.window_cases()
    c = cases["count_across_trips"]
    assert not _same(tc.window_model(c["mem"], c["w"], "state_lost"), c["want"])
    c = cases["enter_count"]
    assert not _same(tc.window_model(c["mem"], c["w"], "entry_state_0"), c["want"])
    c = cases["enter_value_memory_equal"]                           # the memory in front of s0 makes a value look like a repeat
    assert not _same(tc.window_model(c["mem"], c["w"], "prev0_memory"), c["want"])
    assert _same(tc.window_model(c["mem"], c["w"], "prev0_zero"), c["want"])


def test_an_unchecked_exit_accepts_a_flipped_entry():
    c = tc.window_cases()[tc.WINDOW_SMALLEST["exit_unchecked"]]
    for key in ("state1", "prev1"):
        flipped = dict(c["w"], **{key: c["w"][key] ^ 1})
        assert tc.window_model(c["mem"], flipped) is None
        assert _same(tc.window_model(c["mem"], flipped, "exit_unchecked"), c["want"])
    flipped = dict(c["w"], out1=c["w"]["out1"] ^ 1)                 # `out` is held by the carry's own total in either model
    assert tc.window_model(c["mem"], flipped, "exit_unchecked") is None


@pytest.mark.parametrize("variant", tc.DC_VARIANTS)
def test_every_dc_variant_changes_its_smallest_case(variant):
    cases = tc.dc_cases()
    for c in cases.values():
        assert np.array_equal(tc.dc_model(c["expanded"], c["w"]), c["want"])
    c = cases[tc.DC_SMALLEST[variant]]
    assert not np.array_equal(tc.dc_model(c["expanded"], c["w"], variant), c["want"])
    for smaller in tc.DC_SMALLER[variant]:
        s = cases[smaller]
        assert np.array_equal(tc.dc_model(s["expanded"], s["w"], variant), s["want"]), smaller
    far = cases["window_far"]                                       # the 256 parts count from the block that holds out0
    assert not np.array_equal(tc.dc_model(far["expanded"], far["w"], variant), far["want"])


@pytest.mark.parametrize("variant", tc.PLAN_VARIANTS)
def test_every_plan_variant_changes_its_smallest_case(variant):
    cases = tc.plan_cases()
    for raw in cases.values():
        assert tc.plan_model(raw) == len(tc.rle_encode(raw))
    raw = cases[tc.PLAN_SMALLEST[variant]]
    assert tc.plan_model(raw, variant) != len(tc.rle_encode(raw))
    for smaller in tc.PLAN_SMALLER[variant]:
        assert tc.plan_model(cases[smaller], variant) == len(tc.rle_encode(cases[smaller])), smaller
    if variant == "run_before_lost":                                # the run restarts at the trip: one cut fewer, one symbol fewer
        assert tc.plan_model(raw, variant) == len(tc.rle_encode(raw)) - 1


def test_exit_flips_are_refused_by_the_host(ia):
    """what test_gpu_unpack_trips compares the device with: a flipped bit of entry c1 of a stream that leaves behind block 64"""
    for what, bad in tc.far_exit_flips(ia):
        got, _, route = ia.parse_container_window_by_index(tc.container("B"), bad, tc.RECTS["B_span"][1])
        assert route == 1, what
        assert np.array_equal(got, tc.expected_window("B", tc.RECTS["B_span"][1])[0]), what
