"""The seek index the encoder emits, on the host (no GPU): the by-plan route records every checkpoint while it writes the codes,
which defines what the device's code kernel records, and index_from_plan turns the plans and those positions into the blob.
Every equality is exact: the container is assemble_symbol_streams's, the index is container_index's of that container."""
import numpy as np
import pytest

import encode_index_cases as cases
import parse_cases
import stream_cases


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


def _indexed(ia, case, interval):
    return ia.assemble_symbol_streams_by_plan_indexed(case["W"], case["H"], case["K"], 8, case["quant"], case["counts"], case["streams"],
                                                      interval)


def _check(ia, case, want, intervals, name):
    for interval in intervals:
        blob, index = _indexed(ia, case, interval)
        assert blob == want, (name, interval)
        assert index == ia.container_index(want, interval), (name, interval, cases.first_difference(ia, index, ia.container_index(want, interval)))


def test_the_case_covers_what_it_is_meant_to(ia):
    blob = cases.check_coverage(ia)
    assert cases.assemble(ia, cases.main(), by_plan=True) == blob


def test_by_plan_index_equals_the_parsed_index(ia):
    main = cases.main()
    _check(ia, main, cases.assemble(ia, main), cases.INTERVALS, "main")
    for name in ("C", "D"):
        _check(ia, cases.synthetic(name), parse_cases.synthetic()[name], (0, 33, 4096), name)


def test_the_reference_container(ia, mn_bytes):
    # from_container asserts first that the streams read back code to the file itself
    _check(ia, cases.from_container(ia, mn_bytes), mn_bytes, (0, 32, 33, 4097), "mn")


def test_inconsistent_streams_get_no_index(ia):
    c = stream_cases.make()
    q = stream_cases.quant(c["K"])
    want = ia.assemble_symbol_streams(c["W"], c["H"], c["K"], 8, q, c["counts"], c["as_coded"])
    with pytest.raises(ia.MpcError):
        ia.container_index(want)
    blob, index = ia.assemble_symbol_streams_by_plan_indexed(c["W"], c["H"], c["K"], 8, q, c["counts"], c["as_coded"], 128)
    assert blob == want and index is None


def test_bad_intervals(ia):
    main = cases.main()
    for interval in (1, 31, 65537, -5):
        with pytest.raises(ia.MpcError) as e:
            _indexed(ia, main, interval)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    assert ia.index_info(_indexed(ia, main, 0)[1])["interval"] == 128
