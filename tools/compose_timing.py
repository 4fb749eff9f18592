#!/usr/bin/env python3
"""compose_timing.py -- change a 256x256 corner of a stored frame: composed from the container's symbols and the new pixels, against
the two ways there were before, in one process.
    python tools/compose_timing.py [--workloads raise,1080p] [--runs 20] [--once LEG]
Per workload (bench.py's synthetic frame, seed 12345) a base container with its version-2 index, encoded untimed here, and one 256x256
pixel part (the frame of seed 12346) that lands at the tile-aligned middle of the frame.  Legs:
    a   compose: the base through its index, the pixel part through the tile encode (host pixels, uploaded by the call), one container job
    a'  the same with the pixel part already in device memory
    b   encode_image_device of the edited pixels: what there was for a caller who still holds the original pixels, on the device
    c   decode_images_indexed_device then encode_image_device of the decoded pixels with the patch pasted in: what there was without
        them -- a second lossy generation for every tile, so its bytes differ
a, a' and b give the same bytes, asserted before the clock.  After a warm-up the legs alternate, `runs` times; host clock around calls
that return with the container complete.  Prints median and range in ms.
--once LEG: a warm-up and one pass of that leg on the first workload, nothing else (for a profiler or MPC_TRACE=1)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="raise,1080p")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--once", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    from bench import WORKLOADS, synth_frame
    for workload in args.workloads.split(","):
        W, H, K, q = WORKLOADS[workload]
        ctx = ia.create_compression_context(K, 8, q, device=0)
        frame = synth_frame(W, H, 12345)
        side = 256
        x, y = (W - side) // 16 * 8, (H - side) // 16 * 8
        patch = np.ascontiguousarray(synth_frame(W, H, 12346)[y:y + side, x:x + side])
        edited = frame.copy()
        edited[y:y + side, x:x + side] = patch
        base, index = ctx.encode_images_indexed([frame], 0, expanded=True)[0]
        d_edited = torch.from_numpy(edited).cuda()
        d_patch = torch.from_numpy(patch).cuda()
        d_scratch = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
        parts = [(0, None, 0, 0), (patch, None, x, y)]
        d_parts = [(0, None, 0, 0), ((d_patch.data_ptr(), side, side, 3 * side), None, x, y)]

        def leg_a():
            blob, _, routes = ctx.compose([base], [index], parts, W, H)
            assert routes == [0, 2], routes
            return blob

        def leg_a_device():
            blob, _, routes = ctx.compose([base], [index], d_parts, W, H, device_pixels=True)
            assert routes == [0, 2], routes
            return blob

        def leg_b():
            return ctx.encode_image_device(d_edited.data_ptr(), W, H)

        def leg_c():
            pixels, _ = ctx.decode_images_indexed_device([base], [index], out=[d_scratch])
            pixels[0][y:y + side, x:x + side] = d_patch
            torch.cuda.synchronize()
            return ctx.encode_image_device(pixels[0].data_ptr(), W, H)
        legs = [("a", leg_a, "compose, host pixels"), ("a'", leg_a_device, "compose, device pixels"),
                ("b", leg_b, "encode_image_device of the edited pixels"), ("c", leg_c, "decode_images_indexed_device + encode_image_device")]
        made = bytes(leg_a())
        same = made == bytes(leg_a_device()) == bytes(leg_b())
        print(f"# {workload}: {W}x{H} K={K} quality {q}, base {len(base) / 1e6:.2f} MB, index {len(index) / 1e6:.2f} MB, {side}x{side} pixels at "
              f"({x}, {y}); a, a', b give the same {len(made)} bytes: {same}; c gives the same bytes: {bytes(leg_c()) == made}", flush=True)
        assert same
        if args.once:
            leg = {key: fn for key, fn, _ in legs}[args.once]
            leg()
            torch.cuda.synchronize()
            t = time.perf_counter()
            leg()
            print(f"{workload} {args.once}: {(time.perf_counter() - t) * 1e3:.2f} ms", flush=True)
            ctx.close()
            return
        for _ in range(3):                                           # warm-up: buffers grown, pages touched
            for _, fn, _ in legs:
                fn()
        ms = {key: [] for key, _, _ in legs}
        for _ in range(args.runs):
            for key, fn, _ in legs:
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = fn()
                ms[key].append((time.perf_counter() - t) * 1e3)
                del res
        med = {k: statistics.median(v) for k, v in ms.items()}
        for key, _, label in legs:
            v = ms[key]
            print(f"{workload:6s} {key:2s} {label:52s} {med[key]:8.2f} ms (range {min(v):.2f} - {max(v):.2f})  x{med['b'] / med[key]:.2f} of b", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
