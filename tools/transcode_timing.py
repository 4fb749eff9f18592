#!/usr/bin/env python3
"""transcode_timing.py -- the container of a rectangle of a stored frame: transcoded from the source container's symbols against
every other way to the same or a like container, in one process.
    python tools/transcode_timing.py [--workload raise] [--frames 1,8] [--rounds 5] [--interval 0] [--once LEG --shape SHAPE]
Two sets of n distinct containers of a workload (bench.py's synthetic frames, seeds 12345 + f; the second set with the middle third
of every frame's columns in one colour, the flat band of decode_region_timing.py), encoded with their version-2 indexes untimed
here.  Three shapes: a 1024x1024 interior rectangle, a full-height band 512 wide, the whole frame at steps 8.  Legs:
    a   transcode_views, route 0 with the version-2 index
    b   transcode_views, route 1 (no index)
    c   encode_images of the cropped original pixels: what there was before for the same bytes (the steps-8 shape: a full encode,
        the truncation's time not included)
    d   decode_regions (route 0) then encode_images of the decoded pixels: the generational route, lossy a second time
    e   the steps-only shape: truncate_container on the host
a, b and (for steps 0) c give the same bytes, asserted before the clock.  After a warm-up of every shape the legs alternate, `rounds`
times; host clock around calls that return with the containers complete.  Prints median and range of ms per frame.
--once LEG --shape SHAPE: a warm-up and one pass of that leg over n frames of the first --frames value, nothing else (for a
profiler or MPC_TRACE=1)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="raise")
    ap.add_argument("--frames", default="1,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--interval", type=int, default=0)
    ap.add_argument("--once", default=None)
    ap.add_argument("--shape", default="interior", choices=["interior", "band", "steps"])
    args = ap.parse_args()
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    from bench import WORKLOADS, synth_frame
    counts = [int(v) for v in args.frames.split(",")]
    W, H, K, q = WORKLOADS[args.workload]
    ctx = ia.create_compression_context(K, 8, q, device=0)
    n_max = max(counts)
    side = min(1024, (W // 8) * 8, (H // 8) * 8)
    band = min(512, (W // 8) * 8)
    steps = min(8, K)
    shapes = {"interior": (((W - side) // 16 * 8, (H - side) // 16 * 8, side, side), 0), "band": (((W - band) // 16 * 8, 0, band, H), 0),
              "steps": ((0, 0, W, H), steps)}
    for flat in (False, True):
        def frame(f):
            rgb = synth_frame(W, H, 12345 + f)
            if flat:
                rgb = rgb.copy()
                rgb[:, W // 3:2 * W // 3] = (90, 140, 200)
            return rgb
        frames = [frame(f) for f in range(n_max)]
        pairs = ctx.encode_images_indexed(frames, args.interval)
        containers = [p[0] for p in pairs]
        indexes = [ia.index_extend(b, x) for b, x in pairs]
        name = args.workload + (" flat band" if flat else "")
        print(f"# {name}: {W}x{H} K={K} quality {q}, {n_max} containers, {sum(len(b) for b in containers) / n_max / 1e6:.2f} MB each", flush=True)
        for shape, (rect, m) in shapes.items():
            x, y, w, h = rect
            crops = [np.ascontiguousarray(f[y:y + h, x:x + w]) for f in frames]

            def leg_a(n):
                out, routes = ctx.transcode_views(containers[:n], indexes[:n], [(rect, m, 0)] * n)
                assert not any(routes), routes
                return out

            def leg_b(n):
                out, routes = ctx.transcode_views(containers[:n], [None] * n, [(rect, m, 0)] * n)
                assert all(routes), routes
                return out

            def leg_c(n):
                return ctx.encode_images(crops[:n])

            def leg_d(n):
                pixels, routes = ctx.decode_regions(containers[:n], indexes[:n], [rect] * n)
                return ctx.encode_images(pixels)

            def leg_e(n):
                return [ia.truncate_container(b, m) for b in containers[:n]]
            legs = [("a", leg_a, "transcode_views, version-2 index"), ("b", leg_b, "transcode_views, no index"),
                    ("c", leg_c, "encode_images of the cropped pixels"), ("d", leg_d, "decode_regions + encode_images")]
            if m:
                legs.append(("e", leg_e, "truncate_container (host)"))
            same = leg_a(1) == leg_b(1) and (m != 0 or leg_a(1) == leg_c(1)) and (m == 0 or leg_a(1) == leg_e(1))
            print(f"# {name} {shape}: rectangle {rect} steps {m}: {len(leg_a(1)[0])} bytes; a, b{', c' if m == 0 else ', e'} give the same "
                  f"bytes: {same}", flush=True)
            assert same
            if args.once:
                if shape != args.shape:
                    continue
                n, leg = counts[0], {key: fn for key, fn, _ in legs}[args.once]
                leg(n)
                torch.cuda.synchronize()
                t = time.perf_counter()
                leg(n)
                print(f"{name} {shape} {args.once} n={n}: {(time.perf_counter() - t) * 1e3 / n:.2f} ms/frame", flush=True)
                continue
            for n in counts:
                for _, fn, _ in legs:                                # warm-up of every shape: buffers grown, pages touched
                    fn(n)
                ms = {key: [] for key, _, _ in legs}
                for _ in range(args.rounds):
                    for key, fn, _ in legs:
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        res = fn(n)
                        ms[key].append((time.perf_counter() - t) * 1e3 / n)
                        del res
                med = {k: statistics.median(v) for k, v in ms.items()}
                for key, _, label in legs:
                    v = ms[key]
                    print(f"{name} {shape:8s} n={n:2d} {key} {label:36s} {med[key]:8.2f} ms/frame (range {min(v):.2f} - {max(v):.2f})  "
                          f"x{med['c'] / med[key]:.2f} of c", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
