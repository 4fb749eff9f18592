#!/usr/bin/env python3
"""record_budget_hashes.py -- what mpc_encode_image_budget returns for the frames of tests/quality_cases.py, as JSON:
    MPCODEC_LIB=<a build of the commit to record> python tools/record_budget_hashes.py --out tests/golden/budget_bytes_parent.json
tests/test_gpu_target_quality.py holds the budget encode to the file, which was written with the library of the commit in front of the
target-quality encode: that pull request must not change a byte of what the budget encode returns.  Needs a GPU."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import imageexperiments_amd as ia
    import quality_cases as qc
    from oracle import oracle_py as O
    O.build(ref=False)
    contexts = {}

    def context(K, fast):
        if (K, fast) not in contexts:
            contexts[K, fast] = ia.create_compression_context(K, 8, 3.5, device=0).set_fast(fast)
        return contexts[K, fast]

    got = qc.budget_golden(context, O.synth_frame, hashlib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(version=ia.load_library().mpc_version().decode(), entries=got), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} entries -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
