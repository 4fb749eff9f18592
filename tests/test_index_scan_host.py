"""The seek index from a bit scan, on the host (no GPU): mpc_container_index_scan -- step table, segment maps, chain and walk per
stream, the proposal accepted by the chunked parse -- against the serial builder.  For every input the status, the error text and
the blob are mpc_container_index2's, byte for byte; the scan may give up (route 1) only where the serially built index is not one
the chunked parse uses.  The small segment and window sizes make codes span several segments (D's unary runs, C's 20-bit codes
against 32-bit segments) and streams span many windows."""
import pytest

import parse_cases
from container_cases import corpus as _corpus
from parse_cases import INTERVALS

SIZES = ((0, 0), (32, 64), (64, 4096), (256, 1024), (4096, 4096))      # (segment_bits, window_bits); 0 = the library's defaults
# of container_cases.corpus's 768 damaged containers, those whose serially built index the chunked parse uses: counted on the CPU
CORPUS_ROUTE_0 = 363


@pytest.fixture(scope="module")
def ia():
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module")
def cases(ia, oracle):
    """[(name, container)] of A - E"""
    return list(parse_cases.synthetic().items()) + parse_cases.real(oracle)


@pytest.mark.parametrize("sizes", SIZES)
def test_scan_equals_the_serial_builder(ia, cases, sizes):
    for name, blob in cases:
        for interval in INTERVALS:
            for flags in (0, ia.api.MPC_INDEX_EXPANDED):
                got, route = ia.container_index_scan(blob, interval, flags, *sizes)
                assert route == 0, (name, interval, flags)
                assert got == ia.container_index2(blob, interval, flags), (name, interval, flags)


def test_golden_frame(ia):
    mn = parse_cases.golden_mn()
    got, route = ia.container_index_scan(mn)
    assert route == 0 and got == ia.container_index(mn)


def test_damaged_containers(ia, oracle):
    """status, error text and blob are the serial builder's for all 768 damaged containers, and the scan gives up on none whose
    serially built index parse_container_by_index takes route 0 with: 363 of the 768 (counted here, on the CPU; the other 405 are
    refused by the serial parser itself or have an index the chunked parse does not use).  A scan that always gave up could not pass."""
    scanned = must = total = 0
    for n, blob, xs in _corpus(oracle):
        for k, x in enumerate(xs):
            total += 1
            flags = k % 2
            sizes = SIZES[k % len(SIZES)]
            try:
                want = ia.container_index2(x, parse_cases.EDGE_INTERVAL, flags)
            except ia.MpcError as e:
                with pytest.raises(ia.MpcError) as mine:
                    ia.container_index_scan(x, parse_cases.EDGE_INTERVAL, flags, *sizes)
                assert (mine.value.status, str(mine.value)) == (e.status, str(e)), (n, k)
                continue
            got, route = ia.container_index_scan(x, parse_cases.EDGE_INTERVAL, flags, *sizes)
            assert got == want, (n, k)
            assert route in (0, 1)
            if ia.parse_container_by_index(x, want)[1] == 0:
                must += 1
                assert route == 0, (n, k)
            scanned += route == 0
    assert total == 768
    assert scanned == must == CORPUS_ROUTE_0


def test_refused_arguments(ia):
    blob = parse_cases.synthetic()["B"]
    bad = [dict(interval=i) for i in (1, 31, 65537, -5)] + [dict(flags=f) for f in (2, 3, 0x80000000)]
    bad += [dict(segment_bits=s, window_bits=w) for s, w in ((16, 64), (31, 4096), (65536, 65536), (64, 32), (64, 96), (32, 1 << 27), (-1, 64),
                                                             (64, -1))]
    for kwargs in bad:
        with pytest.raises(ia.MpcError) as e:
            ia.container_index_scan(blob, **kwargs)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, kwargs
