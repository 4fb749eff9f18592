"""The frame pipeline with several frames per pursuit launch (MPC_SEQ_GROUP) against the oracle's encodeImage (run with -m gpu).

Every case is a fresh child process with the environment set (the library reads its switches per call, but the pipeline's slots
and streams are made once per context), one child after another.  K = 8, quality 3.5, bench.synth_frame; 70x37 frames are ragged in
both directions (9 x 5 tiles, rows of 210 bytes: the byte path), 328x200 frames have rows of 984 bytes (the 8-byte path).  The
sequence lengths cover a group cut short by the end of the call (3, 5, 9, 13 at two frames per launch; 1, 2, 5, 13 at three),
fewer frames than a group (1, 2), more frames than the pipeline has slots (9) and two wraps of the slots (13).  The `mixed` child
runs both routes and both sizes in turn on one context (MIXED)."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = ((70, 37), (328, 200))
LENGTHS = (1, 2, 3, 5, 9, 13)
DISTINCT = 7                                   # distinct frames in turn: neither the slots (6) nor a group (2, 3) divide it
# device-pointer sequences: a frame number, or 100 + a frame number = that frame copied to an odd byte offset inside a larger tensor
DEVICE_CASES = {
    "distinct": [i % DISTINCT for i in range(13)],
    "twice": [0, 0, 1, 1, 1, 2, 0, 0],         # the same pointer twice in one launch, at two and at three frames per launch
    "odd": [0, 103, 2, 103, 104, 5, 101],      # one frame of a launch off the 8-byte grid: the whole launch reads bytes
    "odd_first": [103],
}
# calls on one context, in order: (route, frames, width, height).  The host and the device layouts of a slot differ by the image at
# its front, and the two sizes by everything: every call carves the slots anew
MIXED = (("host", 1, 70, 37), ("device", 13, 328, 200), ("host", 5, 328, 200), ("device", 2, 70, 37), ("indexed", 3, 70, 37))

_CHILD = r"""
import sys, hashlib, json
sys.path.insert(0, {root!r})
import numpy as np
import imageexperiments_amd as ia
from bench import synth_frame
mode, sizes, lengths, distinct, device_cases, mixed = json.loads(sys.argv[1])
h = lambda b: hashlib.sha256(bytes(b)).hexdigest()
ctx = ia.create_compression_context(8, 8, 3.5, device=0)
if mode.startswith("fast"):
    ctx.set_fast(True)
out = {{}}
if mode == "mixed":                            # one context, the calls of `mixed` in order: the slots are carved anew between them
    import torch
    sizes, out = [], []
    for route, n, W, H in mixed:
        fr = [synth_frame(W, H, 12345 + f % distinct) for f in range(n)]
        if route == "host":
            got = ctx.encode_images(fr)
        elif route == "indexed":
            got = [b for b, x in ctx.encode_images_indexed(fr, interval=32)]
        else:
            d = [torch.from_numpy(f).cuda() for f in fr]
            torch.cuda.synchronize()
            got = ctx.encode_images_device([t.data_ptr() for t in d], W, H)
        out.append([h(b) for b in got])
for W, H in sizes:
    fr = [synth_frame(W, H, 12345 + f) for f in range(distinct)]
    seq = lambda n: [fr[i % distinct] for i in range(n)]
    res = {{}}
    if mode in ("host", "fast_host"):
        for n in lengths:
            res[str(n)] = [h(b) for b in ctx.encode_images(seq(n))]
    elif mode in ("device", "fast_device"):
        import torch
        d = [torch.from_numpy(f).cuda() for f in fr]
        odd = []
        for f in fr:
            big = torch.zeros(f.size + 64, dtype=torch.uint8, device="cuda")
            big[1:1 + f.size] = torch.from_numpy(f).cuda().reshape(-1)
            assert (big.data_ptr() + 1) % 2 == 1
            odd.append(big)
        torch.cuda.synchronize()
        for name, ids in device_cases.items():
            ptrs = [odd[i - 100].data_ptr() + 1 if i >= 100 else d[i].data_ptr() for i in ids]
            res[name] = [h(b) for b in ctx.encode_images_device(ptrs, W, H)]
    elif mode == "indexed":
        import torch
        d = [torch.from_numpy(f).cuda() for f in fr]
        for expanded in (False, True):
            got = ctx.encode_images_indexed(seq(9), interval=32, expanded=expanded)
            res["host v%d" % (2 if expanded else 1)] = [[h(b), h(x)] for b, x in got]
            got = ctx.encode_images_indexed_device([d[i % distinct].data_ptr() for i in range(9)], W, H, interval=32, expanded=expanded)
            res["device v%d" % (2 if expanded else 1)] = [[h(b), h(x)] for b, x in got]
    out["%dx%d" % (W, H)] = res
print(json.dumps(out))
"""


def run_child(mode, env, sizes=SIZES):
    spec = json.dumps([mode, sizes, LENGTHS, DISTINCT, DEVICE_CASES, MIXED])
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), spec], capture_output=True, text=True, timeout=600,
                       env={**os.environ, **env})
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def want(oracle):
    """sha256 of the oracle's container of every distinct frame, per size"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    from bench import synth_frame
    octx = oracle.OracleContext(8, 8, 3.5)
    return {f"{W}x{H}": [hashlib.sha256(octx.encode_image(synth_frame(W, H, 12345 + f))).hexdigest() for f in range(DISTINCT)]
            for W, H in SIZES}


@pytest.mark.parametrize("group", (1, 2, 3))
def test_host_frames_equal_the_oracle(want, group):
    got = run_child("host", {"MPC_SEQ_GROUP": str(group)})
    for size, gold in want.items():
        for n in LENGTHS:
            assert got[size][str(n)] == [gold[i % DISTINCT] for i in range(n)], (size, n, group)


@pytest.mark.parametrize("group", (1, 2, 3))
def test_device_frames_equal_the_oracle(want, group):
    got = run_child("device", {"MPC_SEQ_GROUP": str(group)})
    for size, gold in want.items():
        for name, ids in DEVICE_CASES.items():
            assert got[size][name] == [gold[i % 100] for i in ids], (size, name, group)


def test_default_group_equals_the_oracle(want):
    """no switch set: whatever the library groups by default, on both routes"""
    got = run_child("device", {})
    for size, gold in want.items():
        assert got[size]["distinct"] == [gold[i] for i in DEVICE_CASES["distinct"]], size
    got = run_child("host", {}, sizes=SIZES[1:])
    assert got["328x200"]["13"] == [want["328x200"][i % DISTINCT] for i in range(13)]


@pytest.mark.parametrize("group", (None, 3))
def test_routes_and_sizes_mixed_on_one_context_equal_the_oracle(want, group):
    got = run_child("mixed", {} if group is None else {"MPC_SEQ_GROUP": str(group)})
    assert len(got) == len(MIXED)
    for (route, n, W, H), hashes in zip(MIXED, got):
        assert hashes == [want[f"{W}x{H}"][i % DISTINCT] for i in range(n)], (route, n, W, H, group)


def test_indexed_encoders_in_groups_equal_frame_by_frame(want):
    one = run_child("indexed", {"MPC_SEQ_GROUP": "1"})
    two = run_child("indexed", {"MPC_SEQ_GROUP": "2"})
    assert two == one
    for size, gold in want.items():
        for name, pairs in two[size].items():
            assert [p[0] for p in pairs] == [gold[i % DISTINCT] for i in range(9)], (size, name)


def test_host_entropy_route_in_groups(want):
    got = run_child("host", {"MPC_SEQ_GROUP": "2", "MPC_HOST_ENTROPY": "1"})
    for size, gold in want.items():
        for n in LENGTHS:
            assert got[size][str(n)] == [gold[i % DISTINCT] for i in range(n)], (size, n)


@pytest.mark.parametrize("mode", ("fast_host", "fast_device"))
def test_float_flavour_in_groups_equals_frame_by_frame(mode):
    """the float flavour has no oracle bytes here: equality with one frame per launch is the condition"""
    one = run_child(mode, {"MPC_SEQ_GROUP": "1"})
    two = run_child(mode, {"MPC_SEQ_GROUP": "2"})
    assert two == one
    assert len(set(one["328x200"]["13" if mode == "fast_host" else "distinct"])) == DISTINCT     # not thirteen times the same thing
