#!/usr/bin/env python3
"""emphasis_timing.py -- the two measurements behind profiles/emphasis_encode.txt, one GPU visit each.
    python tools/emphasis_timing.py --leg neutral --parent-lib ab_libs/parent/libmpcodec.so [--runs 12]
    python tools/emphasis_timing.py --leg gain
neutral  "the neutral path costs nothing": encode_image_budget_device (budget: half the full container) and encode_image_quality_device
         (the full container's PSNR minus 2 dB) at 4928x3264, K = 32, quality 3.5, bench.py's frame, on --parent-lib's library (a build
         of the commit in front of this feature, loaded beside this one) and on this one, alternated call by call after two warm-up
         calls each, host clock around calls that return with the container complete.  The yardstick is the parent; the margin is the
         spread of the parent's own repeats.  Beside it the three changed kernels alone (the memset of the totals and the one launch,
         HIP events, buffers of their own) on both libraries.
gain     "what the feature buys": the natural frame of tests/golden (the .jpg), K = 32, a budget of half the full container, the map 64
         in the central quarter and 8 outside: the PSNR of the emphasised tiles and of the rest from distortion_device's per-tile
         squared error of the records cut to the returned depths, with the map and with none; the two sizes and multipliers; and
         emphasis_from_mask_device on a 4928x3264 mask against a device-to-device copy of the same bytes."""
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

W, H, K = 4928, 3264, 32


def _us(torch, fn, n=12, warm=2):
    out = []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b) * 1e3)
    return f"{statistics.median(out):7.1f} us ({min(out):.1f} - {max(out):.1f})"


def neutral_leg(runs, parent_lib):
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
    assert parent.L is other and new.L is not other and not hasattr(other, "mpc_encode_image_budget_emphasis")
    d_rgb = torch.from_numpy(synth_frame(np, W, H, 12345)).cuda()
    tiles = -(-W // 8) * -(-H // 8)
    torch.cuda.synchronize()
    full = new.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=(1 << 64) - 1)
    budget = full.full_bytes // 2
    target = 20.0 * math.log10(765.0) - 10.0 * math.log10(full.full_sse / (W * H)) - 2.0
    print(f"{W}x{H} K={K}: full container {full.full_bytes} bytes; budget {budget}; target PSNR {target:.3f} dB", flush=True)
    calls = {"budget": lambda c: c.encode_image_budget_device(d_rgb.data_ptr(), W, H, budget),
             "quality": lambda c: c.encode_image_quality_device(d_rgb.data_ptr(), W, H, psnr=target)}
    for what, call in calls.items():
        ms = {"parent": [], "new": []}
        got = {}
        for i in range(2 + runs):
            for side, c in (("parent", parent), ("new", new)):        # alternated call by call
                torch.cuda.synchronize()
                t = time.perf_counter()
                got[side] = call(c)
                took = (time.perf_counter() - t) * 1e3
                if i >= 2:
                    ms[side].append(took)
        assert got["parent"].container == got["new"].container and got["parent"].lambda_index == got["new"].lambda_index
        p, n = ms["parent"], ms["new"]
        spread = max(p) - min(p)
        diff = statistics.median(n) - statistics.median(p)
        print(f"  {what:8s} parent {_span(p)}   new {_span(n)}   median new - parent {diff:+.3f} ms, the parent's own spread {spread:.3f} ms: "
              f"{'no change' if abs(diff) <= spread else 'OUTSIDE the spread'}; the same bytes, multiplier {got['new'].lambda_index}", flush=True)
    # the three changed kernels alone, on both libraries
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    d_profile = torch.zeros((tiles, K + 1), dtype=torch.int32, device="cuda")
    d_sweep = torch.zeros((256, 3), dtype=torch.int64, device="cuda")
    d_depth, d_send = torch.zeros(tiles, dtype=torch.uint8, device="cuda"), torch.zeros(tiles, dtype=torch.uint8, device="cuda")
    d_cut = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_e = torch.randint(1, 65, (tiles,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    new.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, -(-H // 8), d_counts.data_ptr(), d_choices.data_ptr(), stream=stream)
    new.depth_profile_device(d_counts.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), W, H, d_profile.data_ptr(), stream=stream)
    weights = ia.budget_weights(ia.container_index(new.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), W, H, stream=stream)))
    j = 100
    for side, c in (("parent", parent), ("new", new)):
        print(f"  kernels, {side}: allocate " + _us(torch, lambda: c.budget_allocate_device(d_profile.data_ptr(), d_counts.data_ptr(), tiles, weights, j, d_depth.data_ptr(),
                                                                                           d_cut.data_ptr(), d_totals.data_ptr(), stream=stream)) +
              "   sweep " + _us(torch, lambda: c.budget_sweep_device(d_profile.data_ptr(), d_counts.data_ptr(), tiles, weights, d_sweep.data_ptr(), stream=stream)) +
              "   floor allocate " + _us(torch, lambda: c.budget_allocate_floor_device(d_profile.data_ptr(), d_counts.data_ptr(), 0, 0, tiles, weights, j, d_depth.data_ptr(),
                                                                                      d_cut.data_ptr(), d_send.data_ptr(), d_totals.data_ptr(), stream=stream)), flush=True)
    print("  kernels, new, with a map: allocate " +
          _us(torch, lambda: new.budget_allocate_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e.data_ptr(), tiles, weights, j, d_depth.data_ptr(),
                                                                 d_cut.data_ptr(), d_totals.data_ptr(), stream=stream)) +
          "   sweep " + _us(torch, lambda: new.budget_sweep_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), d_e.data_ptr(), tiles, weights, d_sweep.data_ptr(),
                                                                            stream=stream)) +
          "   floor allocate " + _us(torch, lambda: new.budget_allocate_floor_emphasis_device(d_profile.data_ptr(), d_counts.data_ptr(), 0, 0, d_e.data_ptr(), 0, tiles, tiles,
                                                                                             weights, j, d_depth.data_ptr(), d_cut.data_ptr(), d_send.data_ptr(),
                                                                                             d_totals.data_ptr(), stream=stream)), flush=True)
    parent.close()
    new.close()


def gain_leg():
    import numpy as np
    import torch
    from PIL import Image
    import imageexperiments_amd as ia
    rgb = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "r0c1de5e1t.jpg")).convert("RGB"), np.uint8)
    h, w = rgb.shape[:2]
    tiles_x, tiles_y = -(-w // 8), -(-h // 8)
    tiles = tiles_x * tiles_y
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    d_rgb = torch.from_numpy(rgb).cuda()
    # the map from a pixel mask: 255 in the central quarter of the frame (half its width, half its height)
    mask = np.zeros((h, w), np.uint8)
    mask[h // 4:h - h // 4, w // 4:w - w // 4] = 255
    d_mask, d_e = torch.from_numpy(mask).cuda(), torch.zeros(tiles, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.emphasis_from_mask_device(d_mask.data_ptr(), w, h, d_e.data_ptr(), lo=8, hi=64)
    torch.cuda.synchronize()
    e = d_e.cpu().numpy()
    assert np.array_equal(e, ia.emphasis_from_mask(mask, 8, 64)) and set(e.tolist()) == {8, 64}
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_tiles_device(d_rgb.data_ptr(), w, h, 3 * w, 0, tiles_y, d_counts.data_ptr(), d_choices.data_ptr())
    torch.cuda.synchronize()
    full = bytes(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), w, h))
    budget = len(full) // 2
    # pixels of each tile inside the frame
    tx, ty = np.divmod(np.arange(tiles), tiles_y)
    pixels = np.minimum(8, w - tx * 8) * np.minimum(8, h - ty * 8)
    inside = e == 64

    def psnr(sse, n):
        return float("inf") if sse == 0 else 20.0 * math.log10(765.0) - 10.0 * math.log10(sse / n)

    print(f"natural frame {w}x{h}, K={K}: full container {len(full)} bytes, budget {budget}; {int(inside.sum())} of {tiles} tiles at 64, the rest at 8", flush=True)
    for label, got in (("no map", ctx.encode_image_budget_device(d_rgb.data_ptr(), w, h, budget)),
                       ("with the map", ctx.encode_image_budget_emphasis_device(d_rgb.data_ptr(), w, h, budget, d_e.data_ptr()))):
        cut = torch.minimum(d_counts.to(torch.int32), torch.from_numpy(got.depth.astype(np.int32)).cuda()[:, None]).to(torch.int16).contiguous()
        d_sse, d_tile = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(tiles, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.distortion_device(cut.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), w, h, d_sse.data_ptr(), d_tile.data_ptr())
        torch.cuda.synchronize()
        tile = d_tile.cpu().numpy().astype(np.int64)
        assert int(tile.sum()) == int(d_sse[0]) == got.sse
        print(f"  {label:13s} {len(got.container)} bytes at multiplier {got.lambda_index} ({got.probes} probes): PSNR of the emphasised tiles "
              f"{psnr(int(tile[inside].sum()), int(pixels[inside].sum())):.3f} dB, of the rest {psnr(int(tile[~inside].sum()), int(pixels[~inside].sum())):.3f} dB, "
              f"of the frame {psnr(got.sse, w * h):.3f} dB", flush=True)
    # the mask kernel against a copy of the same bytes
    big = torch.randint(0, 256, (H, W), dtype=torch.uint8, device="cuda")
    copy = torch.empty_like(big)
    out = torch.zeros(-(-W // 8) * -(-H // 8), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    print(f"  emphasis_from_mask_device, {W}x{H} mask ({W * H} bytes): " + _us(torch, lambda: ctx.emphasis_from_mask_device(big.data_ptr(), W, H, out.data_ptr(), stream=stream)) +
          "   a device-to-device copy of the same bytes: " + _us(torch, lambda: copy.copy_(big)), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=("neutral", "gain"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--parent-lib", default=None, help="a build of the commit in front of the emphasis maps")
    args = ap.parse_args()
    if args.leg == "neutral":
        if not args.parent_lib:
            ap.error("--leg neutral needs --parent-lib")
        neutral_leg(args.runs, args.parent_lib)
    else:
        gain_leg()
    return 0


if __name__ == "__main__":
    sys.exit(main())
