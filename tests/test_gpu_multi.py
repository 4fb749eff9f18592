"""mpc_encode_images_multi: several device lanes driven from ONE process (the C++ side of SURVEY 8e).  A one-GPU box offers one
device, so every lane names device 0 (one context per lane): stripes, peer copies, interleave and the pipelined container jobs are
the real code, only the copies stay on one device.  Every container must equal the oracle's whole-frame encodeImage, in either
flavour; lanes that would put stripes of two encoders (flavours, quantiser tables) into one container are refused."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from pursuit_cases import fine_table

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X")
    return torch


@pytest.mark.parametrize("lanes,frames,size,K", [(2, 3, (200, 136), 32), (3, 4, (97, 83), 8), (2, 1, (70, 50), 32), (4, 9, (64, 40), 16)])
def test_lanes_on_one_device_reproduce_the_oracles_bytes(gpu, oracle, lanes, frames, size, K):
    import imageexperiments_amd as ia
    W, H = size
    ctxs = [ia.create_compression_context(K, 8, 3.5, device=0) for _ in range(lanes)]
    rgbs = [oracle.synth_frame(W, H, 4000 + f) for f in range(frames)]
    octx = oracle.OracleContext(K, 8, 3.5)
    for rep in range(2):                                       # twice: a second call allocates and pipelines afresh
        blobs = ia.api.encode_images_multi(ctxs, rgbs)
        assert len(blobs) == frames
        for f in range(frames):
            assert bytes(blobs[f]) == bytes(octx.encode_image(rgbs[f])), (rep, f)
    # the quantiser override of a call reaches every lane
    q = np.ones((3, K))
    blobs = ia.api.encode_images_multi(ctxs, rgbs[:2], quant=q)
    for f in range(min(2, frames)):
        assert bytes(blobs[f]) == bytes(octx.encode_image(rgbs[f], quant=q))


@pytest.mark.parametrize("lanes,frames,size,K", [(2, 3, (200, 136), 32), (3, 4, (97, 83), 8)])
def test_float_lanes_reproduce_the_float_oracles_bytes(gpu, oracle, lanes, frames, size, K):
    """all lanes float (mpc_context_set_fast): the containers are oracle/mpo_fast.c's.  With the context's tables the two oracles
    agree on these frames, so the call is repeated with pursuit_cases.fine_table, with which every tile row differs between the
    flavours (tests/test_pursuit_cases.py): every lane's stripe provably comes from the float kernel."""
    import imageexperiments_amd as ia
    W, H = size
    ctxs = [ia.create_compression_context(K, 8, 3.5, device=0).set_fast(True) for _ in range(lanes)]
    rgbs = [oracle.synth_frame(W, H, 4000 + f) for f in range(frames)]
    octx = oracle.OracleContext(K, 8, 3.5)
    of = oracle.OracleFastContext(octx)
    want = [bytes(of.encode_image(r)) for r in rgbs]
    for rep in range(2):
        blobs = ia.api.encode_images_multi(ctxs, rgbs)
        assert [bytes(b) for b in blobs] == want, rep
    q = fine_table(K)
    want = [bytes(of.encode_image(r, quant=q)) for r in rgbs]
    assert all(w != bytes(octx.encode_image(r, quant=q)) for w, r in zip(want, rgbs))
    blobs = ia.api.encode_images_multi(ctxs, rgbs, quant=q)
    assert [bytes(b) for b in blobs] == want
    for c in ctxs:
        c.close()


def test_lanes_of_different_flavour_or_tables_are_refused(gpu, oracle):
    """A frame's stripes meet in one container whose header carries the owner's tables.  Lanes that differ in flavour, or (no table
    given with the call) in their own quantiser tables, would mix two encoders in it: MPC_ERR_ARGUMENT, nothing encoded.  An
    explicit table makes different context tables harmless: allowed, and every lane uses it."""
    import imageexperiments_amd as ia
    K, W, H = 8, 97, 83
    rgbs = [oracle.synth_frame(W, H, 4000 + f) for f in range(3)]
    octx = oracle.OracleContext(K, 8, 3.5)
    of = oracle.OracleFastContext(octx)
    a, b, c = (ia.create_compression_context(K, 8, 3.5, device=0) for _ in range(3))
    for fast_flags in ((False, True), (True, False), (False, False, True), (True, False, True)):
        lanes = [a, b, c][:len(fast_flags)]
        for ctx, fast in zip(lanes, fast_flags):
            ctx.set_fast(fast)
        with pytest.raises(ia.MpcError) as e:
            ia.api.encode_images_multi(lanes, rgbs)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT, fast_flags
    # the refusal leaves the contexts usable, in either flavour
    fine = fine_table(K)                                                # every tile row shows its flavour with this table
    for fast, o in ((True, of), (False, octx)):
        for ctx in (a, b, c):
            ctx.set_fast(fast)
        assert [bytes(x) for x in ia.api.encode_images_multi([a, b, c], rgbs)] == [bytes(o.encode_image(r)) for r in rgbs]
        assert [bytes(x) for x in ia.api.encode_images_multi([a, b, c], rgbs, quant=fine)] == [bytes(o.encode_image(r, quant=fine)) for r in rgbs]
    # different bpp_allocation, quant=None: refused; with an explicit table: the oracle's bytes for that table
    other = ia.create_compression_context(K, 8, 5.0, device=0)
    assert (other.quant != a.quant).any()
    for lanes in ([a, other], [other, a], [a, b, other]):
        with pytest.raises(ia.MpcError) as e:
            ia.api.encode_images_multi(lanes, rgbs)
        assert e.value.status == ia.api.MPC_ERR_ARGUMENT
    q = oracle.OracleContext(K, 8, 2.0).quant
    blobs = ia.api.encode_images_multi([a, other, b], rgbs, quant=q)
    assert [bytes(x) for x in blobs] == [bytes(octx.encode_image(r, quant=q)) for r in rgbs]
    # a table set on the context later (Compression.cpp's "max" mode) counts like the one it was created with
    other.set_quant(a.quant)
    assert [bytes(x) for x in ia.api.encode_images_multi([a, other], rgbs)] == [bytes(octx.encode_image(r)) for r in rgbs]
    for ctx in (a, b, c, other):
        ctx.close()


def test_more_lanes_than_tile_rows_is_refused(gpu, oracle):
    import imageexperiments_amd as ia
    ctxs = [ia.create_compression_context(8, 8, 3.5, device=0) for _ in range(3)]
    with pytest.raises(ia.MpcError):
        ia.api.encode_images_multi(ctxs, [oracle.synth_frame(40, 16, 1)])      # two tile rows, three lanes
    with pytest.raises(ia.MpcError):
        ia.api.encode_images_multi([ctxs[0], ctxs[0]], [oracle.synth_frame(40, 40, 1)])   # one context in two lanes


def test_configs3_frames_at_full_size_through_two_lanes(gpu):
    """BASELINE configs[3]'s first frames (4928x3264, K = 32, quality 3.5, seeds 12345 + f) striped over two lanes: golden sha256."""
    import imageexperiments_amd as ia
    import bench
    with open(os.path.join(ROOT, "tests", "golden", "frames.json")) as f:
        gold = json.load(f)
    ctxs = [ia.create_compression_context(32, 8, 3.5, device=0) for _ in range(2)]
    rgbs = [bench.synth_frame(4928, 3264, 12345 + f) for f in range(3)]
    blobs = ia.api.encode_images_multi(ctxs, rgbs, views=True)
    for f, name in enumerate(("raise_k32_q3.5", "batch_frame1_k32_q3.5", "batch_frame2_k32_q3.5")):
        assert len(blobs[f]) == gold[name]["container_bytes"]
        assert hashlib.sha256(np.ascontiguousarray(blobs[f]).tobytes()).hexdigest() == gold[name]["container_sha256"], name
