"""Index version 2 as the encoder emits it, on the host (no GPU): the by-plan route computes the aux entries from the coded streams
it holds (index_aux_pass), which defines what the device's pack pass and sum kernels compute, and index_from_plan turns plans,
checkpoints and entries into the blob.  Every equality is exact: the container is assemble_symbol_streams's, the index is
container_index(container, interval, expanded=True), which is also what index_extend makes of the version-1 index."""
import pytest

import encode_index2_cases as cases
import stream_cases


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def _indexed(ia, case, interval, expanded=True):
    return ia.assemble_symbol_streams_by_plan_indexed(case["W"], case["H"], case["K"], 8, case["quant"], case["counts"], case["streams"],
                                                      interval, expanded=expanded)


def test_the_cases_cover_what_they_are_meant_to(ia):
    cases.check_coverage(ia)


@pytest.mark.parametrize("name", cases.NAMES)
def test_by_plan_index_equals_the_parsed_and_the_extended_index(ia, name):
    case, want = cases.case(name), cases.container(name)
    for interval in cases.INTERVALS:
        blob, index = _indexed(ia, case, interval)
        assert blob == want, (name, interval)
        parsed = ia.container_index(want, interval, expanded=True)
        assert ia.index_version(index) == 2, (name, interval)
        assert index == parsed, (name, interval, cases.first_difference(ia, index, parsed))
        v1 = ia.container_index(want, interval)
        assert index == ia.index_extend(want, v1), (name, interval)
        blob, plain = _indexed(ia, case, interval, expanded=False)
        assert blob == want and plain == v1, (name, interval)


def test_no_entries_is_still_version_2(ia):
    """a frame without a single record: no stream has an aux entry, and the blob is the (empty) version-2 one"""
    import numpy as np
    case = dict(W=16, H=8, K=2, quant=np.ones((3, 2)), counts=np.zeros(6, np.uint16), streams=[np.zeros(0, np.uint16)] * 12)
    want = cases.assemble(ia, case)
    blob, index = _indexed(ia, case, 32)
    assert blob == want and ia.index_version(index) == 2 and index == ia.container_index(want, 32, expanded=True)


def test_flags_zero_is_the_version_1_call(ia):
    import ctypes as C
    import numpy as np
    from imageexperiments_amd import api
    case = cases.case("main2")
    L = ia.load_library()
    q = np.ascontiguousarray(case["quant"], np.float64).reshape(-1)
    counts = np.ascontiguousarray(case["counts"], np.uint16)
    symbols = np.concatenate(case["streams"]).astype(np.uint16)
    off = np.zeros(6 * case["K"] + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in case["streams"]])

    def call(flags, interval=100):
        out, n, idx, ni = api._u8p(), C.c_size_t(0), api._u8p(), C.c_size_t(0)
        st = L.mpc_assemble_symbol_streams_by_plan_indexed2(case["W"], case["H"], case["K"], 8, q.ctypes.data_as(api._dp),
                                                            counts.ctypes.data_as(api._u16p), symbols.ctypes.data_as(api._u16p),
                                                            off.ctypes.data_as(C.POINTER(C.c_ulonglong)), interval, flags, C.byref(out),
                                                            C.byref(n), C.byref(idx), C.byref(ni))
        if st != api.MPC_OK:
            assert not out and not idx
            return st, None, None
        return st, api._take_bytes(L, out, n), api._take_bytes(L, idx, ni)
    want = cases.container("main2")
    assert call(0) == (api.MPC_OK, want, ia.container_index(want, 100))
    assert call(api.MPC_INDEX_EXPANDED) == (api.MPC_OK, want, ia.container_index(want, 100, expanded=True))
    for flags in (2, 3, 4, 0x80000000, 0x80000001):
        assert call(flags)[0] == api.MPC_ERR_ARGUMENT, flags
    for interval in (1, 31, 65537, -5):
        assert call(api.MPC_INDEX_EXPANDED, interval)[0] == api.MPC_ERR_ARGUMENT, interval


def test_inconsistent_streams_get_no_index(ia):
    c = stream_cases.make()
    q = stream_cases.quant(c["K"])
    want = ia.assemble_symbol_streams(c["W"], c["H"], c["K"], 8, q, c["counts"], c["as_coded"])
    blob, index = ia.assemble_symbol_streams_by_plan_indexed(c["W"], c["H"], c["K"], 8, q, c["counts"], c["as_coded"], 128, expanded=True)
    assert blob == want and index is None


def test_bad_intervals(ia):
    main2 = cases.main2()
    for interval in (1, 31, 65537, -5):
        with pytest.raises(ia.MpcError) as e:
            _indexed(ia, main2, interval)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    assert ia.index_info(_indexed(ia, main2, 0)[1])["interval"] == 128
