"""A fixed slice of the fuzzers inside the suite (run with -m gpu).

tools/fuzz_parity.py hunts with fresh seeds and tosses a coin for the flavour; here a fixed seed gives 48 random small frames
(tests/pursuit_cases.py: fuzz_frames) and BOTH flavours run on every one: container bytes equal the matching oracle's, decoded
pixels equal the matching oracle decoder's.  tools/fuzz_streams.py's generator (tests/stream_cases.py: fuzz_streams) gives 12
random sets of symbol streams for the device-side entropy stage against the oracle's writeCompressed."""
import numpy as np
import pytest

import pursuit_cases
import stream_cases

pytestmark = pytest.mark.gpu

FRAME_SEED, FRAME_CASES = 20241016, 48
STREAM_SEED, STREAM_CASES = 20241017, 12


@pytest.fixture(scope="module")
def ia():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the gpu-marked tests need a real MI355X (there is no CPU fallback)")
    import imageexperiments_amd as ia
    return ia


def test_random_frames_both_flavours_bytes_and_pixels(ia, oracle):
    ctxs, octxs = {}, {}                                              # per (K, bpp), as the tool caches them
    bad, seen = [], set()
    for n, (W, H, K, bpp, kind, rgb) in enumerate(pursuit_cases.fuzz_frames(FRAME_SEED, FRAME_CASES, oracle.synth_frame)):
        assert rgb.shape == (H, W, 3) and W < 200 and H < 160
        key = (K, bpp)
        if key not in ctxs:
            ctxs[key] = ia.create_compression_context(K, 8, bpp, device=0)
            octxs[key] = oracle.OracleContext(K, 8, bpp)
            octxs[key, "fast"] = oracle.OracleFastContext(octxs[key])
        ctx = ctxs[key]
        seen.add(kind)
        for fast in (False, True):
            ctx.set_fast(fast)
            want = (octxs[key, "fast"] if fast else octxs[key]).encode_image(rgb)
            got = ctx.encode_image(rgb)
            ok = got == want
            if ok:
                dec = ia.decode_image(got, ctx)
                ok = bool((dec == (oracle.decode_image_fast(got) if fast else oracle.decode_image(got))).all())
            if not ok:
                bad.append(f"case {n}: {W}x{H} K={K} bpp={bpp} kind={kind} fast={fast}")
    for c in ctxs.values():
        c.close()
    assert seen == {0, 1, 2, 3, 4}                                    # every kind of content is in the slice
    assert not bad, bad


def test_random_symbol_streams_through_the_device_entropy_stage(ia, oracle):
    ctxs, bad = {}, []
    for c, case in enumerate(stream_cases.fuzz_streams(STREAM_SEED, STREAM_CASES)):
        K, W, H = case["K"], case["W"], case["H"]
        want = oracle.write_compressed(dict(W=W, H=H, K=K, bs=8, quant=case["quant"], lengths=case["counts"], codes=case["as_held"]))
        if K not in ctxs:
            ctxs[K] = ia.create_compression_context(K, 8, 3.5, device=0)
        got, route = ctxs[K].code_symbol_streams_device(W, H, case["counts"], case["as_coded"], quant=case["quant"])
        if got != want:
            bad.append(f"case {c}: K={K} {W}x{H} route={route} sizes {[len(x) for x in case['as_held']]}")
    for c in ctxs.values():
        c.close()
    assert not bad, bad
