#!/usr/bin/env python3
"""fuzz_parity.py -- random small frames (sizes, K, quality, content, both flavours) through the product against the oracle:
container bytes and decoded pixels.  A hunting tool; a fixed slice runs in the suite (tests/test_gpu_fuzz_slice.py, both flavours on
every case; the case generator is tests/pursuit_cases.py: fuzz_frames): python tools/fuzz_parity.py [cases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import imageexperiments_amd as ia
    from oracle import oracle_py as O
    import pursuit_cases
    O.build(ref=False)
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    ctxs, octxs = {}, {}
    bad = 0
    for n, (W, H, K, bpp, kind, rgb) in enumerate(pursuit_cases.fuzz_frames(rng, cases, O.synth_frame)):
        fast = bool(rng.integers(0, 2))                          # drawn from the generator's rng between two cases, as before
        key = (K, bpp)
        if key not in ctxs:
            ctxs[key] = ia.create_compression_context(K, 8, bpp, device=0)
            octxs[key] = O.OracleContext(K, 8, bpp)
        ctx, octx = ctxs[key], octxs[key]
        ctx.set_fast(fast)
        want = (O.OracleFastContext(octx) if fast else octx).encode_image(rgb)
        got = ctx.encode_image(rgb)
        ok = got == want
        if ok:
            dec = ia.decode_image(got, ctx)
            ok = bool((dec == (O.decode_image_fast(got) if fast else O.decode_image(got))).all())
        if not ok:
            bad += 1
            print(f"MISMATCH case {n}: {W}x{H} K={K} bpp={bpp} kind={kind} fast={fast}", flush=True)
    print(f"{cases} cases, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
