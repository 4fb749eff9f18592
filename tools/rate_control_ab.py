#!/usr/bin/env python3
"""rate_control_ab.py -- the budget encode, the quality encode and the delta stream to a budget on this library and on another build
of it (the parent commit's), both loaded in one process and alternated call by call; per call the host clock around a call that
returns with its result complete, the parent's median and range beside this library's, and whether the latter's median lies inside
the parent's range.  The bytes of both must agree.
    python tools/rate_control_ab.py --parent-lib <a build of the parent commit> --leg 4928x3264:32 [--stream] [--runs 8]
--stream: the delta stream as well (a key frame, then frames in which a band of 1/8 of the rows changes, to 1/16 of the full container).
Two controls tell a shift of the code from one of the process: --parent-lib given a copy of this library, and the order of the two
sides changed -- --swap calls this library first in every pair, --parent-first creates the parent's context first.  Needs a GPU."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from budget_timing import QUALITY, synth_frame                       # noqa: E402
from quality_timing import _second_library, _span                    # noqa: E402


def verdict(p, n):
    med = statistics.median(n)
    inside = min(p) <= med <= max(p)
    return (f"parent {_span(p)}   new {_span(n)}   new's median {'inside' if inside else 'OUTSIDE'} the parent's range "
            f"({statistics.median(n) - statistics.median(p):+.3f} ms against its median)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--leg", required=True)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--swap", action="store_true", help="call the new library first in every pair")
    ap.add_argument("--parent-first", action="store_true", help="create the parent's context before the new one")
    args = ap.parse_args()
    size, K = args.leg.split(":")
    W, H = (int(v) for v in size.split("x"))
    K = int(K)
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    from imageexperiments_amd import api
    new = None if args.parent_first else ia.create_compression_context(K, 8, QUALITY, device=0)
    other = _second_library(api, args.parent_lib)
    mine, api._lib = api._lib, other
    try:
        parent = ia.create_compression_context(K, 8, QUALITY, device=0)
    finally:
        api._lib = mine
    if new is None:
        new = ia.create_compression_context(K, 8, QUALITY, device=0)
    assert parent.L is other and new.L is not other
    sides = (("new", new), ("parent", parent)) if args.swap else (("parent", parent), ("new", new))
    frame = synth_frame(np, W, H, 12345)
    d_rgb = torch.from_numpy(frame).cuda()
    torch.cuda.synchronize()
    full = new.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=(1 << 64) - 1)
    target = 20.0 * math.log10(765.0) - 10.0 * math.log10(full.full_sse / (W * H)) - 2.0
    print(f"{W}x{H} K={K}: full container {full.full_bytes} bytes; quality target {target:.3f} dB", flush=True)
    calls = {"budget 1/2": lambda c: c.encode_image_budget_device(d_rgb.data_ptr(), W, H, full.full_bytes // 2),
             "budget 1/4": lambda c: c.encode_image_budget_device(d_rgb.data_ptr(), W, H, full.full_bytes // 4),
             "quality": lambda c: c.encode_image_quality_device(d_rgb.data_ptr(), W, H, psnr=target)}
    for what, call in calls.items():
        ms = {"parent": [], "new": []}
        got = {}
        for i in range(2 + args.runs):
            for side, c in sides:
                torch.cuda.synchronize()
                t = time.perf_counter()
                got[side] = call(c)
                took = (time.perf_counter() - t) * 1e3
                if i >= 2:
                    ms[side].append(took)
        assert got["parent"].container == got["new"].container and repr(got["parent"]) == repr(got["new"])
        probes = f", {got['new'].probes} probes" if hasattr(got["new"], "probes") else ""
        print(f"  {what:10s} {verdict(ms['parent'], ms['new'])}; the same bytes, multiplier {got['new'].lambda_index}{probes}", flush=True)
    if args.stream:
        # a key frame at half the full container, then frames whose band of 1/8 of the rows comes from another frame, at 1/16
        sessions = {side: c.delta_encoder(W, H) for side, c in sides}
        other_frame = synth_frame(np, W, H, 54321)
        ms = {"parent": [], "new": []}
        band = H // 8
        for i in range(3 + args.runs):
            cur = frame.copy()
            if i > 0:
                y = (i * band) % (H - band)
                cur[y:y + band] = np.roll(other_frame, i, axis=1)[y:y + band]
            got = {}
            for side, _ in sides:
                torch.cuda.synchronize()
                t = time.perf_counter()
                got[side] = sessions[side].encode_patch_budget(cur, full.full_bytes // 16 if i else full.full_bytes // 2)
                took = (time.perf_counter() - t) * 1e3
                if i >= 3:
                    ms[side].append(took)
            assert got["parent"][0] == got["new"][0] and repr(got["parent"][1]) == repr(got["new"][1])
        print(f"  stream     {verdict(ms['parent'], ms['new'])}; the same patches, last call {got['new'][1]}", flush=True)
        for s in sessions.values():
            s.close()
    parent.close()
    new.close()


if __name__ == "__main__":
    main()
