"""Index version 2 emitted by the encoder on the GPU (run with -m gpu): the pack pass of the entropy stage records out, prev and state
of every interval-th symbol it writes (mp_entropy.hip, ent_runs_kernel<true, true>), ent_dc_kernel adds the sums of the step-0
coefficient streams, the host checks the entries against its plans.  Every equality is exact: the container is the one the call
without an index returns, the index is container_index(container, interval, expanded=True)."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import encode_index2_cases as cases
import index2_cases
import stream_cases
from conftest import ROOT
from container_cases import FRAMES

pytestmark = pytest.mark.gpu

STREAM_INTERVALS = (32, 33, 100, 4096, 65536)
FRAME_INTERVALS = (0, 33)
SHAPES = (2, 11, 7, 1)                              # of container_cases.FRAMES: 200x120 K=32 max, 1003x517 K=8 max, 200x120 K=8 q2, 16x8 K=8
REGION_SHAPE = 11                                   # the 1003x517 one: index2_cases.F2_INNER lies inside


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


@pytest.fixture(scope="module", autouse=True)
def device_dictionary(ia):
    """a context that lives as long as the module: the contexts the tests create and close share its device dictionary
    instead of building one each"""
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module", autouse=True)
def strict():
    """entries the host refuses are an error here, not a quiet parse of the finished container: the blobs compared below are the
    device's own (the child processes of test_host_route inherit it; on the host route it has nothing to say)"""
    before = os.environ.get("MPC_INDEX_STRICT")
    os.environ["MPC_INDEX_STRICT"] = "1"
    yield
    if before is None:
        del os.environ["MPC_INDEX_STRICT"]
    else:
        os.environ["MPC_INDEX_STRICT"] = before


@functools.lru_cache(maxsize=None)
def _parsed(blob, interval, expanded=True):
    import imageexperiments_amd as ia
    return ia.container_index(blob, interval, expanded=expanded)


def _same_index(ia, got, blob, interval, what):
    want = _parsed(blob, interval)
    assert got == want, f"{what}: {cases.first_difference(ia, got, want)}"


@pytest.mark.parametrize("name", ["main2", "main", "f1", "f2", "D"])
def test_streams(ia, name):
    case = cases.case(name)
    if name == "main2":
        cases.check_coverage(ia)
    want = cases.container(name)
    ctx = ia.create_compression_context(case["K"], 8, 3.5, device=0)
    args = (case["W"], case["H"], case["counts"], case["streams"])
    plain, route = ctx.code_symbol_streams_device(*args, quant=case["quant"])
    assert route == 0 and plain == want
    for interval in STREAM_INTERVALS:
        for attempt in range(2):                    # twice on one context, a version-1 call and a call without an index in between
            blob, index, route = ctx.code_symbol_streams_device_indexed(*args, interval=interval, quant=case["quant"], expanded=True)
            assert route == 0, (name, interval, attempt)
            assert blob == plain, (name, interval, attempt)
            _same_index(ia, index, blob, interval, f"{name} at {interval}, call {attempt}")
            blob, v1, route = ctx.code_symbol_streams_device_indexed(*args, interval=interval, quant=case["quant"])
            assert route == 0 and blob == plain and v1 == _parsed(plain, interval, False), (name, interval, attempt)
            between, route = ctx.code_symbol_streams_device(*args, quant=case["quant"])
            assert route == 0 and between == plain, (name, interval, attempt)
    ctx.close()


@pytest.mark.parametrize("fast", [False, True], ids=["double", "fast"])
@pytest.mark.parametrize("shape", SHAPES)
def test_frames(ia, oracle, shape, fast):
    import torch
    W, H, K, quality = FRAMES[shape]
    ctx = ia.create_compression_context(K, 8, 3.5 if quality == "max" else quality, device=0)
    ctx.set_fast(fast)
    quant = np.ones((3, K)) if quality == "max" else None
    frames = [oracle.synth_frame(W, H, 300 + 16 * shape + f) for f in range(9)]        # more than the pipeline's six slots
    d_frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    for n in (1, 9):
        want = ctx.encode_images(frames[:n], quant=quant)
        assert len(set(want)) == n
        for interval in FRAME_INTERVALS:
            for what, got in (("host frames", ctx.encode_images_indexed(frames[:n], interval, quant=quant, expanded=True)),
                              ("device frames", ctx.encode_images_indexed_device([t.data_ptr() for t in d_frames[:n]], W, H, interval,
                                                                                 quant=quant, expanded=True))):
                assert [b for b, _ in got] == want, (what, n, interval)
                for f, (blob, index) in enumerate(got):
                    _same_index(ia, index, blob, interval, f"{what}, frame {f} of {n} at {interval}")
            assert ctx.encode_images(frames[:n], quant=quant) == want              # and a call without an index is what it was
        if shape == REGION_SHAPE:                   # the emitted index cuts the packed and step-0 streams of a region decode
            rect = index2_cases.F2_INNER
            x, y, w, h = rect
            pixels = [np.asarray(p) for p in ctx.decode_images(want)]
            got = ctx.encode_images_indexed(frames[:n], 33, quant=quant, expanded=True)
            regions, routes = ctx.decode_regions([b for b, _ in got], [i for _, i in got], [rect] * n)
            assert routes == [0] * n
            for f, (blob, index) in enumerate(got):
                assert np.array_equal(np.asarray(regions[f]), pixels[f][y:y + h, x:x + w]), (n, f)
                chunks, route = ctx.window_chunks_device(blob, index, rect)
                host_chunks, host_route = ia.window_chunks_by_index(blob, _parsed(blob, 33), rect)
                assert route == 0 and host_route == 0 and np.array_equal(chunks, host_chunks), (n, f)
    ctx.close()


_CHILD = r"""
import sys, hashlib
sys.path.insert(0, {root!r})
import imageexperiments_amd as ia
from bench import synth_frame
ctx = ia.create_compression_context(8, 8, 3.5, device=0)
frames = [synth_frame(328, 200, 12345 + f) for f in range(9)]
for blob, index in ctx.encode_images_indexed(frames, 100, expanded=True):
    print(hashlib.sha256(blob).hexdigest(), hashlib.sha256(index).hexdigest())
"""


def test_host_route(ia):
    """a frame whose entropy stage runs on the host gets its version-2 index from the finished container: the same blob"""
    from bench import synth_frame
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    frames = [synth_frame(328, 200, 12345 + f) for f in range(9)]
    device = ctx.encode_images_indexed(frames, 100, expanded=True)
    assert [b for b, _ in device] == ctx.encode_images(frames)
    want = []
    for blob, index in device:
        assert index == ia.container_index(blob, 100, expanded=True)
        want.append(f"{hashlib.sha256(blob).hexdigest()} {hashlib.sha256(index).hexdigest()}")
    ctx.close()
    for env in ({"MPC_HOST_ENTROPY": "1"}, {"MPC_ENTROPY_TRIPLES": "50"}):
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=600,
                           env={**os.environ, **env})
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().split("\n") == want, env


def _raw_indexed2(ia, ctx, fn, ptrs, n, width, height, interval, flags):
    import ctypes as C
    from imageexperiments_amd import api
    outs, sizes, idx, isizes = (api._u8p * n)(), (C.c_size_t * n)(), (api._u8p * n)(), (C.c_size_t * n)()
    st = fn(ctx.h, ptrs, n, width, height, None, int(interval), int(flags), outs, sizes, idx, isizes)
    if st != api.MPC_OK:
        assert not any(outs[i] for i in range(n)) and not any(idx[i] for i in range(n))
        return st, None
    return st, [(api._take_bytes(ctx.L, outs[i], C.c_size_t(sizes[i])), api._take_bytes(ctx.L, idx[i], C.c_size_t(isizes[i]))) for i in range(n)]


def test_arguments(ia, oracle):
    import ctypes as C
    import torch
    from imageexperiments_amd import api
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    frame = np.ascontiguousarray(oracle.synth_frame(72, 40, 7))
    d_frame = torch.from_numpy(frame).cuda()
    want = ctx.encode_images([frame])
    c = cases.case("D")
    ctx1 = ia.create_compression_context(c["K"], 8, 3.5, device=0)
    host_ptrs = (api._u8p * 1)(frame.ctypes.data_as(api._u8p))
    dev_ptrs = (C.c_void_p * 1)(C.c_void_p(d_frame.data_ptr()))
    calls = ((ctx.L.mpc_encode_images_indexed2, host_ptrs), (ctx.L.mpc_encode_images_indexed2_device, dev_ptrs))
    for flags in (2, 3, 0x100, 0x80000000):         # a bit other than MPC_INDEX_EXPANDED
        for fn, ptrs in calls:
            assert _raw_indexed2(ia, ctx, fn, ptrs, 1, 72, 40, 32, flags)[0] == api.MPC_ERR_ARGUMENT, flags
    for interval in (1, 31, 65537):
        for call in (lambda: ctx.encode_images_indexed([frame], interval, expanded=True),
                     lambda: ctx.encode_images_indexed_device([d_frame.data_ptr()], 72, 40, interval, expanded=True),
                     lambda: ctx1.code_symbol_streams_device_indexed(c["W"], c["H"], c["counts"], c["streams"], interval, quant=c["quant"],
                                                                     expanded=True)):
            with pytest.raises(ia.MpcError) as e:
                call()
            assert e.value.status == api.MPC_ERR_ARGUMENT, interval
    for fn, ptrs in calls:                          # flags == 0: exactly the version-1 call
        st, got = _raw_indexed2(ia, ctx, fn, ptrs, 1, 72, 40, 32, 0)
        assert st == api.MPC_OK and got == [(want[0], ia.container_index(want[0], 32))]
    (blob, index), = ctx.encode_images_indexed([frame], 32, expanded=True)
    assert [blob] == want and index == ia.container_index(blob, 32, expanded=True)
    assert ctx.encode_images([frame]) == want
    ctx.close()
    ctx1.close()


def test_inconsistent_streams(ia):
    c = stream_cases.make()
    q = stream_cases.quant(c["K"])
    ctx = ia.create_compression_context(c["K"], 8, 3.5, device=0)
    want, route = ctx.code_symbol_streams_device(c["W"], c["H"], c["counts"], c["as_coded"], quant=q)
    assert route == 0
    blob, index, route = ctx.code_symbol_streams_device_indexed(c["W"], c["H"], c["counts"], c["as_coded"], 128, quant=q, expanded=True)
    assert blob == want and index is None and route == 0
    ctx.close()
