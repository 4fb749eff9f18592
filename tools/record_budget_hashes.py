#!/usr/bin/env python3
"""record_budget_hashes.py -- what mpc_encode_image_budget returns for the frames of tests/quality_cases.py, as JSON:
    MPCODEC_LIB=<a build of the commit to record> python tools/record_budget_hashes.py --out tests/golden/budget_bytes_parent.json
tests/test_gpu_target_quality.py holds the budget encode to the file, which was written with the library of the commit in front of the
target-quality encode: that pull request must not change a byte of what the budget encode returns.
With --all the other routes through the cut encodes' front end instead -- the quality encode, both encodes with an emphasis map, the
delta stream to a budget (quality_cases.cut_golden):
    MPCODEC_LIB=<...> python tools/record_budget_hashes.py --all --out tests/golden/cut_bytes_parent.json
written with the library of the commit in front of that front end.  Needs a GPU."""
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
    ap.add_argument("--all", action="store_true")
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

    def to_device(array):
        import torch
        tensor = torch.from_numpy(array).cuda()
        torch.cuda.synchronize()
        return tensor

    got = qc.cut_golden(context, O.synth_frame, hashlib, to_device) if args.all else qc.budget_golden(context, O.synth_frame, hashlib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(version=ia.load_library().mpc_version().decode(), entries=got), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} entries -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
