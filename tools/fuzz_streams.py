#!/usr/bin/env python3
"""fuzz_streams.py -- random symbol streams through the device-side entropy stage against the oracle's writeCompressed.
A hunting tool (the generator is tests/stream_cases.py: fuzz_streams; a fixed slice of it runs in the suite,
tests/test_gpu_fuzz_slice.py): python tools/fuzz_streams.py [cases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import imageexperiments_amd as ia
    from oracle import oracle_py as O
    import stream_cases
    O.build(ref=False)
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    ctxs = {}
    bad = 0
    for c, case in enumerate(stream_cases.fuzz_streams(rng, cases)):
        K, W, H, counts, held, coded, q = (case[k] for k in ("K", "W", "H", "counts", "as_held", "as_coded", "quant"))
        want = O.write_compressed(dict(W=W, H=H, K=K, bs=8, quant=q, lengths=counts, codes=held))
        if K not in ctxs:
            ctxs[K] = ia.create_compression_context(K, 8, 3.5, device=0)
        got, route = ctxs[K].code_symbol_streams_device(W, H, counts, coded, quant=q)
        if got != want:
            bad += 1
            print(f"MISMATCH case {c}: K={K} {W}x{H} route={route} sizes {[len(x) for x in held]}", flush=True)
    print(f"{cases} cases, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
