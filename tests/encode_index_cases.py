"""Inputs for the tests of the seek index the encoder emits, shared by the host tests and the device tests (nothing here needs a GPU).

A case is what the entropy stage is handed: dict(W, H, K, quant, counts[3 * tiles], streams[6K]), the streams "as coded" (the step-0
coefficient streams already differenced) and consistent: stream pair (channel, step) holds exactly as many symbols as tiles of
that channel have more atoms than `step`, which is what every parser goes by.

main()            3200 x 2048, K = 4: stream lengths around the entropy stage's 4096-symbol blocks, the run-length cut at 0x8001
                  and the index's intervals; contents cycling through eight kinds
from_container()  the streams of a finished container handed back as coded (parse_cases.case_c / case_d, the reference's .mn)"""
import functools

import numpy as np

import parse_cases
from stream_cases import _dc_difference

W, H, K = 3200, 2048, 4
TILES = (W // 8) * (H // 8)                       # 102 400
# symbols of the stream pairs (channel, step 0 .. 3)
LENGTHS = ((102400, 100000, 0x8003, 0x8001), (12289, 4097, 4096, 4095), (12800, 33, 32, 0))
INTERVALS = (0, 32, 33, 100, 128, 4096, 4097, 65536)
COVERAGE_INTERVAL = 128


def _contents(kind, n, rng):
    if kind == 0:
        return np.zeros(n, np.int64)
    if kind == 1:
        return rng.integers(0, 65536, n)
    if kind == 2:                                                   # short runs
        return np.repeat(rng.integers(0, 50, (n + 3) // 4), 4)[:n]
    if kind == 3:                                                   # wide geometric: a large Golomb M
        return np.minimum(rng.geometric(0.004, n) - 1, 4000)
    if kind == 4:
        return np.full(n, 0xFFFF)
    if kind == 5:
        return np.arange(n) % 30000
    if kind == 6:                                                   # 64 symbols with equal counts: every Huffman tie
        return rng.permutation(np.arange(n) % 64)
    return np.concatenate([np.full(n // 2, 9), np.minimum(rng.geometric(0.3, n - n // 2) - 1, 65535)])


@functools.lru_cache(maxsize=None)
def main():
    rng = np.random.default_rng(20250401)
    counts = np.zeros((TILES, 3), np.int64)
    for ch, lengths in enumerate(LENGTHS):
        assert list(lengths) == sorted(lengths, reverse=True) and lengths[0] <= TILES
        column = np.zeros(TILES, np.int64)
        for n in lengths:                                           # the first n tiles have more atoms than this step
            column[:n] += 1
        counts[:, ch] = rng.permutation(column)
    streams = []
    for i in range(6 * K):
        ch, step = (i // 2) // K, (i // 2) % K
        n = int((counts[:, ch] > step).sum())
        assert n == LENGTHS[ch][step]
        streams.append(np.asarray(_contents(i % 8, n, rng), np.int64).astype(np.uint16))
    return dict(W=W, H=H, K=K, quant=np.ones((3, K)), counts=counts.astype(np.uint16).reshape(-1), streams=streams)


def from_container(ia, blob):
    """a container's streams as its encoder's entropy stage saw them; asserts that coding them gives the container back"""
    s = ia.read_compressed(blob)
    k = s["K"]
    streams = [np.asarray(c, np.uint16) for c in s["codes"]]
    for i in (1, 2 * k + 1, 4 * k + 1):
        streams[i] = _dc_difference(streams[i]) if len(streams[i]) else streams[i]
    case = dict(W=s["W"], H=s["H"], K=k, quant=s["quant"].astype(np.float64), counts=s["lengths"], streams=streams)
    assert s["bs"] == 8 and assemble(ia, case) == bytes(blob), "the streams read back do not code to the container they came from"
    return case


def assemble(ia, case, by_plan=False):
    return ia.assemble_symbol_streams(case["W"], case["H"], case["K"], 8, case["quant"], case["counts"], case["streams"], by_plan=by_plan)


@functools.lru_cache(maxsize=None)
def synthetic(name):
    """parse_cases' C (a Huffman table 20 bits deep) and D (Golomb unary parts of about 240 bits) as stream cases"""
    import imageexperiments_amd as ia
    return from_container(ia, parse_cases.synthetic()[name])


def check_coverage(ia):
    """what main() is there for, read from its container's index"""
    blob = assemble(ia, main())
    info = ia.index_info(ia.container_index(blob, COVERAGE_INTERVAL))
    assert not info["serial_only"]
    streams = info["streams"]
    assert {s["mode"] for s in streams} == {0, 1}
    assert {s["packed"] for s in streams[1:]} == {True, False}
    sizes = [s["n_coded"] for s in streams]
    assert 0 in sizes
    assert any(0 < n < COVERAGE_INTERVAL for n in sizes)
    assert any(n and n % COVERAGE_INTERVAL == 0 for n in sizes)
    assert [s["expect"] for s in streams[1:]] == [LENGTHS[(i // 2) // K][(i // 2) % K] for i in range(6 * K)]
    _, route = ia.parse_container_by_index(blob, ia.container_index(blob, COVERAGE_INTERVAL))
    assert route == 0
    return blob


def first_difference(ia, got, want):
    """where two indexes of one container differ, for an assertion's message"""
    if got == want:
        return "equal"
    if got is None or want is None:
        return f"one is missing: got {None if got is None else len(got)} bytes, want {None if want is None else len(want)}"
    try:
        a, b = ia.index_info(got), ia.index_info(want)
    except ia.MpcError as e:
        return f"not an index: {e}"
    for key in ("interval", "serial_only", "nbytes", "W", "H", "K", "bs"):
        if a[key] != b[key]:
            return f"header field {key}: {a[key]} against {b[key]}"
    for j, (x, y) in enumerate(zip(a["streams"], b["streams"])):
        for key in ("mode", "m", "packed", "n_coded", "expect", "wrapper_bit", "end_bit"):
            if x[key] != y[key]:
                return f"stream {j} field {key}: {x[key]} against {y[key]}"
        if len(x["checkpoints"]) != len(y["checkpoints"]):
            return f"stream {j}: {len(x['checkpoints'])} checkpoints against {len(y['checkpoints'])}"
        bad = np.nonzero(x["checkpoints"] != y["checkpoints"])[0]
        if bad.size:
            return f"stream {j} checkpoint {bad[0]}: bit {x['checkpoints'][bad[0]]} against {y['checkpoints'][bad[0]]}"
    return f"sizes {len(got)} against {len(want)}, fields equal"
