#!/usr/bin/env python3
"""group_budget_timing.py -- the measurement behind profiles/group_budget.txt, one GPU visit.
    python tools/group_budget_timing.py --parent-lib ab_libs/parent/libmpcodec.so [--runs 8] [--out profiles/group_budget.txt]
Groups of 4 and 8 frames of mixed content (crops of the photograph of tests/golden, a flat frame, a noisy frame) at 1920x1080 K = 8 and
4928x3264 K = 32, quality 3.5, the frames in device memory.  Budgets of 1/2 and 1/4 of the full containers' bytes, quality targets of the
full containers' PSNR over the whole group minus 1 and minus 3 dB.  For each: encode_images_budget_device / encode_images_quality_device
on this library, median (range) of --runs calls after two warm-ups, and beside it the n single-frame calls -- budget / n each, or each
frame's own full squared error times the same factor, which adds up to the group's target -- on --parent-lib's library (a build of the commit in front of this feature, loaded beside this one), alternated call
by call in one process, host clock around calls that return with the containers complete.  For both: total bytes, total squared error,
bytes per frame.  And the two group kernels alone (the memset of their totals and their launches, HIP events) beside n launches of the
single-frame kernels on the same records."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from budget_timing import QUALITY                                     # noqa: E402
from emphasis_timing import _us                                       # noqa: E402
from quality_timing import _second_library, _span                     # noqa: E402

SPREAD = 0.04                                                         # run to run


def group_frames(np, W, H, n):
    """n frames of W x H: crops of the photograph at different places (the photograph rolled sideways, every other one upside down, where
    the crop is its size or the places run out), with a flat frame second and a noisy frame fourth"""
    from PIL import Image
    photo = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "r0c1de5e1t.jpg")).convert("RGB"), np.uint8)
    PH, PW = photo.shape[:2]
    rng = np.random.default_rng(2024)
    out = []
    for k in range(n):
        if k == 1:
            out.append(np.full((H, W, 3), 96, np.uint8))
        elif k == 3:
            out.append(rng.integers(0, 256, (H, W, 3)).astype(np.uint8))
        else:
            x, y = (k * 733) % (PW - W + 1), (k * 419) % (PH - H + 1)
            crop = photo[y:y + H, x:x + W]
            out.append(np.ascontiguousarray(np.roll(crop[::-1] if k % 2 else crop, k * 211, axis=1) if k >= 4 or (W, H) == (PW, PH) else crop))
    return out


def measure(W, H, K, n, runs, parent_lib, say):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    from imageexperiments_amd import api
    new = ia.create_compression_context(K, 8, QUALITY, device=0)
    other = _second_library(api, parent_lib)
    mine, api._lib = api._lib, other
    try:
        parent = ia.create_compression_context(K, 8, QUALITY, device=0)
    finally:
        api._lib = mine
    assert parent.L is other and new.L is not other and not hasattr(other, "mpc_encode_images_budget")
    frames = group_frames(np, W, H, n)
    d_frames = [torch.from_numpy(f).cuda() for f in frames]
    ptrs = [d.data_ptr() for d in d_frames]
    torch.cuda.synchronize()
    full = new.encode_images_quality_device(ptrs, W, H, max_sse=(1 << 64) - 1)
    total, full_sse = full.info.full_bytes, full.info.full_sse
    full_psnr = 20.0 * math.log10(765.0) - 10.0 * math.log10(full_sse / (n * W * H))
    say(f"{n} frames of {W}x{H}, K = {K}: full containers {total} bytes ({', '.join(str(g.full_bytes) for g in full)}), PSNR over the group {full_psnr:.3f} dB")
    legs = [(f"budget 1/{d}", "budget", total // d) for d in (2, 4)] + [(f"quality -{d} dB", "quality", full_psnr - d) for d in (1, 3)]
    for label, kind, target in legs:
        if kind == "budget":
            group = lambda: new.encode_images_budget_device(ptrs, W, H, target)
            singles = lambda: [parent.encode_image_budget_device(p, W, H, target // n) for p in ptrs]
        else:
            loss = 10.0 ** ((full_psnr - target) / 10.0)               # the same loss for every frame: the even split of the group's target
            group = lambda: new.encode_images_quality_device(ptrs, W, H, max_sse=int(full_sse * loss))
            singles = lambda: [parent.encode_image_quality_device(p, W, H, max_sse=int(g.full_sse * loss)) for p, g in zip(ptrs, full)]
        ms = {"group": [], "singles": []}
        got = {}
        for i in range(2 + runs):
            for side, call in (("singles", singles), ("group", group)):   # alternated call by call
                torch.cuda.synchronize()
                t = time.perf_counter()
                try:
                    got[side] = call()
                except ia.MpcError as e:
                    got[side] = e
                took = (time.perf_counter() - t) * 1e3
                if i >= 2:
                    ms[side].append(took)
        g, s = got["group"], got["singles"]
        if isinstance(g, Exception) or isinstance(s, Exception):
            say(f"  {label}: group {g if isinstance(g, Exception) else 'ok'}; singles {s if isinstance(s, Exception) else 'ok'}")
            continue
        ratio = statistics.median(ms["group"]) / statistics.median(ms["singles"])
        verdict = "within" if ratio <= 1.0 + 2 * SPREAD else "OUTSIDE"
        say(f"  {label}: group {_span(ms['group'])}   {n} single calls on the parent {_span(ms['singles'])}   ratio {ratio:.3f}: {verdict} twice the "
            f"+-{SPREAD:.0%} spread")
        say(f"    group:   multiplier {g.info.lambda_index}, {g.size} bytes ({', '.join(str(len(f.container)) for f in g)}), squared error {g.info.sse}"
            + (f", {g.info.probes} probes" if kind == "budget" else ""))
        say(f"    singles: multipliers {[f.lambda_index for f in s]}, {sum(len(f.container) for f in s)} bytes ({', '.join(str(len(f.container)) for f in s)}), "
            f"squared error {sum(f.sse for f in s)}" + (f", {sum(f.probes for f in s)} probes" if kind == "budget" else ""))
        say(f"    squared error, group / singles: {g.info.sse / max(sum(f.sse for f in s), 1):.4f}; bytes, group / singles: {g.size / sum(len(f.container) for f in s):.4f}")
    # the two group kernels alone beside n launches of the single-frame kernels, on records of their own
    tiles = -(-W // 8) * -(-H // 8)
    d_counts = torch.zeros((n, tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((n, tiles, 3, K), dtype=torch.int32, device="cuda")
    d_profile = torch.zeros((n, tiles, K + 1), dtype=torch.int32, device="cuda")
    d_depth, d_cut = torch.zeros((n, tiles), dtype=torch.uint8, device="cuda"), torch.zeros((n, tiles, 3), dtype=torch.int16, device="cuda")
    d_totals, d_sweep = torch.zeros((n, 3), dtype=torch.int64, device="cuda"), torch.zeros((256, 3), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    weights = np.zeros((n, 3, K), np.uint32)
    for f in range(n):
        new.encode_tiles_device(ptrs[f], W, H, 3 * W, 0, -(-H // 8), d_counts[f].data_ptr(), d_choices[f].data_ptr(), stream=stream)
        new.depth_profile_device(d_counts[f].data_ptr(), d_choices[f].data_ptr(), ptrs[f], W, H, d_profile[f].data_ptr(), stream=stream)
        weights[f] = ia.budget_weights(ia.container_index(new.records_to_container_device(d_counts[f].data_ptr(), d_choices[f].data_ptr(), W, H, stream=stream)))
    j = 100
    say("  kernels: group allocate " +
        _us(torch, lambda: new.budget_allocate_group_device(d_profile.data_ptr(), d_counts.data_ptr(), 0, n, tiles, weights, j, d_depth.data_ptr(), d_cut.data_ptr(),
                                                            d_totals.data_ptr(), stream=stream)) +
        f"   {n} single allocates " +
        _us(torch, lambda: [new.budget_allocate_device(d_profile[f].data_ptr(), d_counts[f].data_ptr(), tiles, weights[f], j, d_depth[f].data_ptr(), d_cut[f].data_ptr(),
                                                       d_totals[f].data_ptr(), stream=stream) for f in range(n)]))
    say("  kernels: group sweep    " +
        _us(torch, lambda: new.budget_sweep_group_device(d_profile.data_ptr(), d_counts.data_ptr(), 0, n, tiles, weights, d_sweep.data_ptr(), stream=stream)) +
        f"   {n} single sweeps    " +
        _us(torch, lambda: [new.budget_sweep_device(d_profile[f].data_ptr(), d_counts[f].data_ptr(), tiles, weights[f], d_sweep.data_ptr(), stream=stream)
                            for f in range(n)]))
    parent.close()
    new.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=True, help="a build of the commit in front of the group encodes")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_budget.txt"))
    ap.add_argument("--only", default=None, help="WxH, to measure one geometry")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("group_budget_timing.py: a group call on this library beside n single-frame calls on the parent's, alternated; "
        f"median (range) of {args.runs} after two warm-ups; the frames in device memory")
    for W, H, K in ((1920, 1080, 8), (4928, 3264, 32)):
        if args.only and args.only != f"{W}x{H}":
            continue
        for n in (4, 8):
            measure(W, H, K, n, args.runs, args.parent_lib, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
