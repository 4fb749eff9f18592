"""The seek index emitted by the encoder on the GPU (run with -m gpu): the code-writing kernel of the entropy stage records the
checkpoints (mp_entropy.hip, ent_code_kernel<true, true>), the host adds what it planned.  Every equality is exact: the container
is the one the call without an index returns, the index is container_index's of that container."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import encode_index_cases as cases
import stream_cases
from conftest import ROOT
from container_cases import FRAMES

pytestmark = pytest.mark.gpu

STREAM_INTERVALS = (32, 33, 100, 128, 4096, 4097, 65536)
FRAME_INTERVALS = (0, 33, 4096)
SHAPES = (2, 11, 7, 1)                              # of container_cases.FRAMES: 200x120 K=32 max, 1003x517 K=8 max, 200x120 K=8 q2, 16x8 K=8


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


def _same_index(ia, got, blob, interval, what):
    want = ia.container_index(blob, interval)
    assert got == want, f"{what}: {cases.first_difference(ia, got, want)}"


@pytest.mark.parametrize("name", ["main", "C", "D"])
def test_streams(ia, name):
    case = cases.main() if name == "main" else cases.synthetic(name)
    if name == "main":
        cases.check_coverage(ia)
    want = cases.assemble(ia, case)
    ctx = ia.create_compression_context(case["K"], 8, 3.5, device=0)
    args = (case["W"], case["H"], case["counts"], case["streams"])
    plain, route = ctx.code_symbol_streams_device(*args, quant=case["quant"])
    assert route == 0 and plain == want
    for interval in STREAM_INTERVALS:
        for attempt in range(2):                    # twice on one context, a call without an index in between
            blob, index, route = ctx.code_symbol_streams_device_indexed(*args, interval=interval, quant=case["quant"])
            assert route == 0, (name, interval, attempt)
            assert blob == plain, (name, interval, attempt)
            _same_index(ia, index, blob, interval, f"{name} at {interval}, call {attempt}")
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
        pixels = [np.asarray(x) for x in ctx.decode_images(want)]
        for interval in FRAME_INTERVALS:
            for what, got in (("host frames", ctx.encode_images_indexed(frames[:n], interval, quant=quant)),
                              ("device frames", ctx.encode_images_indexed_device([t.data_ptr() for t in d_frames[:n]], W, H, interval,
                                                                                 quant=quant))):
                assert [b for b, _ in got] == want, (what, n, interval)
                for f, (blob, index) in enumerate(got):
                    _same_index(ia, index, blob, interval, f"{what}, frame {f} of {n} at {interval}")
                decoded, routes = ctx.decode_images_indexed([b for b, _ in got], [x for _, x in got])
                assert routes == [0] * n, (what, n, interval)
                for a, b in zip(decoded, pixels):
                    assert np.array_equal(np.asarray(a), b), (what, n, interval)
            assert ctx.encode_images(frames[:n], quant=quant) == want              # and a call without an index is what it was
    ctx.close()


_CHILD = r"""
import sys, hashlib
sys.path.insert(0, {root!r})
import imageexperiments_amd as ia
from bench import synth_frame
ctx = ia.create_compression_context(8, 8, 3.5, device=0)
frames = [synth_frame(328, 200, 12345 + f) for f in range(9)]
for blob, index in ctx.encode_images_indexed(frames, 100):
    print(hashlib.sha256(blob).hexdigest(), hashlib.sha256(index).hexdigest())
"""


def test_host_route(ia):
    """a frame whose entropy stage runs on the host gets its index from the finished container: the same blob"""
    from bench import synth_frame
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    frames = [synth_frame(328, 200, 12345 + f) for f in range(9)]
    device = ctx.encode_images_indexed(frames, 100)
    assert [b for b, _ in device] == ctx.encode_images(frames)
    want = []
    for blob, index in device:
        assert index == ia.container_index(blob, 100)
        want.append(f"{hashlib.sha256(blob).hexdigest()} {hashlib.sha256(index).hexdigest()}")
    ctx.close()
    for env in ({"MPC_HOST_ENTROPY": "1"}, {"MPC_ENTROPY_TRIPLES": "50"}):
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=600,
                           env={**os.environ, **env})
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().split("\n") == want, env


def test_arguments(ia, oracle):
    import torch
    ctx = ia.create_compression_context(8, 8, 3.5, device=0)
    frame = oracle.synth_frame(72, 40, 7)
    d_frame = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    want = ctx.encode_images([frame])
    c = cases.synthetic("D")
    ctx1 = ia.create_compression_context(1, 8, 3.5, device=0)
    for interval in (1, 31, 65537, -5):
        for call in (lambda: ctx.encode_images_indexed([frame], interval),
                     lambda: ctx.encode_images_indexed_device([d_frame.data_ptr()], 72, 40, interval),
                     lambda: ctx1.code_symbol_streams_device_indexed(c["W"], c["H"], c["counts"], c["streams"], interval, quant=c["quant"])):
            with pytest.raises(ia.MpcError) as e:
                call()
            assert e.value.status == ia.api.MPC_ERR_ARGUMENT, interval
    (blob, index), = ctx.encode_images_indexed([frame], 32)
    assert [blob] == want and index == ia.container_index(blob, 32)
    assert ctx.encode_images([frame]) == want
    ctx.close()
    ctx1.close()


def test_inconsistent_streams(ia):
    c = stream_cases.make()
    q = stream_cases.quant(c["K"])
    ctx = ia.create_compression_context(c["K"], 8, 3.5, device=0)
    want, route = ctx.code_symbol_streams_device(c["W"], c["H"], c["counts"], c["as_coded"], quant=q)
    assert route == 0
    blob, index, route = ctx.code_symbol_streams_device_indexed(c["W"], c["H"], c["counts"], c["as_coded"], 128, quant=q)
    assert blob == want and index is None and route == 0
    ctx.close()
