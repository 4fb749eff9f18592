"""The seek index on the host (no GPU): its structure, the chunked parse that defines what the device parse computes, and the
rule that an index is a hint only: whatever it holds, the result is the serial parse's."""
import numpy as np
import pytest

import parse_cases
from container_cases import corpus as _corpus
from parse_cases import INTERVALS


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def cases(ia, oracle):
    """[(name, container)] of A - E"""
    return list(parse_cases.synthetic().items()) + parse_cases.real(oracle) + [("mn", parse_cases.golden_mn())]


def test_cases_cover_what_they_are_meant_to(ia):
    parse_cases.check_coverage(ia)
    a = parse_cases.synthetic()["A"]
    s = ia.read_compressed(a, coded=True)
    # about 50 KB, 6 of its 24 streams run-length packed
    assert (s["W"], s["H"], s["K"]) == (640, 480, 4) and sum(s["packed"]) == 6 and 50000 <= len(a) < 56000
    whole = ia.read_compressed(a)
    assert [len(c) for c in whole["codes"]] == s["expect"]


def test_index_structure(ia, cases):
    for name, blob in cases:
        s = ia.read_compressed(blob, coded=True)
        sizes = [len(s["lengths"])] + [len(c) for c in s["codes"]]
        for interval in INTERVALS:
            index = ia.container_index(blob, interval)
            assert ia.container_index(blob, interval) == index, name
            info = ia.index_info(index)
            assert (info["interval"], info["serial_only"], info["nbytes"]) == (interval, False, len(blob)), name
            assert (info["W"], info["H"], info["K"], info["bs"]) == (s["W"], s["H"], s["K"], s["bs"]), name
            streams = info["streams"]
            assert len(streams) == 1 + 6 * s["K"]
            assert [x["n_coded"] for x in streams] == sizes, name
            assert [x["packed"] for x in streams[1:]] == s["packed"] and not streams[0]["packed"], name
            assert [x["expect"] for x in streams[1:]] == s["expect"] and streams[0]["expect"] == sizes[0], name
            for j, x in enumerate(streams):
                cp = x["checkpoints"].astype(np.int64)
                assert len(cp) == -(-x["n_coded"] // interval), (name, j)
                assert (np.diff(cp) > 0).all() and (len(cp) == 0 or (x["wrapper_bit"] < cp[0] and cp[-1] < x["end_bit"])), (name, j)
                if j + 1 < len(streams):
                    assert x["end_bit"] == streams[j + 1]["wrapper_bit"], (name, j)
            assert 8 * (len(blob) - 1) < streams[-1]["end_bit"] <= 8 * len(blob), name
            if 2 * interval <= 65536:
                twice = ia.index_info(ia.container_index(blob, 2 * interval))["streams"]
                for j, x in enumerate(streams):
                    assert np.array_equal(twice[j]["checkpoints"], x["checkpoints"][::2]), (name, j)
        assert ia.index_info(ia.container_index(blob))["interval"] == ia.index_info(ia.container_index(blob, 0))["interval"]
    for interval in (1, 31, 65537, -5):
        with pytest.raises(ia.MpcError) as e:
            ia.container_index(cases[0][1], interval)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT


def test_parse_by_index_equals_the_serial_parse(ia, cases):
    for name, blob in cases:
        want, _ = parse_cases.serial(blob)
        for interval in INTERVALS:
            got, route = ia.parse_container_by_index(blob, ia.container_index(blob, interval))
            assert route == 0, (name, interval)
            assert np.array_equal(got, want), (name, interval)


def test_a_damaged_index_changes_nothing(ia, oracle, cases):
    """route 0 is allowed only where the output is still equal, which the acceptance rule guarantees; some damage must be refused"""
    others = dict(list(parse_cases.synthetic(1).items()) + parse_cases.real(oracle, seed=150))
    for n, (name, blob) in enumerate(cases):
        want, _ = parse_cases.serial(blob)
        index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
        # the golden frame has no twin: the index of its own container at another interval stands in
        other = ia.container_index(others[name], parse_cases.EDGE_INTERVAL) if name in others else ia.container_index(blob, 64)
        routes = {"flip": [], "header flip": [], "cut": [], "another": []}
        for what, bad in parse_cases.damaged_indexes(index, other, n):
            got, route = ia.parse_container_by_index(blob, bad)
            assert route in (0, 1), (name, what)
            assert np.array_equal(got, want), (name, what, route)
            routes[next(k for k in routes if what.startswith(k))].append(route)
        assert [len(v) for v in routes.values()] == [64, 16, 16, 1], name
        assert sum(routes["flip"]) >= 1 and all(routes["cut"]), (name, routes)


def test_damaged_containers_with_the_original_index(ia, oracle):
    n_ok = n_refused = 0
    for n, blob, xs in _corpus(oracle):
        index = ia.container_index(blob, parse_cases.EDGE_INTERVAL)
        for x in xs:
            try:
                s = ia.read_compressed(x, coded=True)
            except ia.MpcError as e:
                with pytest.raises(ia.MpcError) as mine:
                    ia.parse_container_by_index(x, index)
                assert (mine.value.status, str(mine.value)) == (e.status, str(e))
                with pytest.raises(ia.MpcError) as built:
                    ia.container_index(x)
                assert built.value.status == ia.api.MPC_ERR_BITSTREAM
                n_refused += 1
                continue
            got, route = ia.parse_container_by_index(x, index)
            assert route in (0, 1)
            assert np.array_equal(got, np.concatenate([s["lengths"]] + s["codes"])), n
            ia.index_info(ia.container_index(x))
            n_ok += 1
    assert n_ok + n_refused == 768 and n_ok > 100 and n_refused > 100
