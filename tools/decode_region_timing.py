#!/usr/bin/env python3
"""decode_region_timing.py -- a pixel rectangle of a frame through its seek index against the whole frame, in one process.
    python tools/decode_region_timing.py [--workloads raise,1080p] [--frames 1,16] [--rounds 5] [--interval 0] [--flat] [--once]
For n distinct containers of a workload (bench.py's: synthetic frames, seeds 12345 + f, encoded with their indexes untimed here):
    a  decode_images_indexed_device     (the whole frame, pixels left in device memory: the baseline of b)
    b  decode_regions_device            for a centred 512x512 rectangle, a full-height band 512 wide, and the whole frame
    c  decode_images_indexed            (the whole frame, host pixels: the baseline of d)
    d  decode_regions                   for the same three rectangles
    b2, d2                              b and d with the version-2 index (index_extend of the encoder's index, made before the clock):
                                        run-length packed and step-0 coefficient streams cut as well
b and d take the encoder's version-1 index.  --flat paints the middle third of every frame's columns in one colour (content with
flat areas: more run-length packed streams).  Also printed: the indexes' sizes, how many of the 6K streams are packed, and the
host's time for index_extend against container_index(expanded=True).
Output buffers are allocated before the clock.  After a warm-up of every shape the legs alternate, `rounds` times; host clock
around calls that return with the pixels complete.  Prints median and range of ms per frame and each against its baseline.
--once: a warm-up and one pass of leg b over n frames of the first --frames value with one rectangle (--rect centre, band or
whole) and the index version of --index-version, nothing else (for MPC_TRACE=1)."""
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
    ap.add_argument("--frames", default="1,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--interval", type=int, default=0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--rect", default="centre", choices=["centre", "band", "whole"])
    ap.add_argument("--index-version", type=int, default=1, choices=[1, 2])
    ap.add_argument("--flat", action="store_true")
    args = ap.parse_args()
    import torch
    import imageexperiments_amd as ia
    from bench import WORKLOADS, synth_frame
    counts = [int(v) for v in args.frames.split(",")]
    for name in args.workloads.split(","):
        W, H, K, q = WORKLOADS[name]
        ctx = ia.create_compression_context(K, 8, q, device=0)
        n_max = max(counts)
        pairs = []

        def frame(f):
            rgb = synth_frame(W, H, 12345 + f)
            if args.flat:
                rgb = rgb.copy()
                rgb[:, W // 3:2 * W // 3] = (90, 140, 200)
            return rgb
        for lo in range(0, n_max, 8):                              # encoded eight at a time: 8 x 48 MB of frames in host memory
            pairs += ctx.encode_images_indexed([frame(f) for f in range(lo, min(n_max, lo + 8))], args.interval)
        containers, indexes = [p[0] for p in pairs], [p[1] for p in pairs]
        t = time.perf_counter()
        indexes2 = [ia.index_extend(b, x) for b, x in zip(containers, indexes)]
        extend_ms = (time.perf_counter() - t) * 1e3 / n_max
        t = time.perf_counter()
        built = ia.container_index(containers[0], ia.index_info(indexes[0])["interval"], expanded=True)
        build_ms = (time.perf_counter() - t) * 1e3
        assert built == indexes2[0]
        packed = sum(1 for s in ia.index_info(indexes[0])["streams"][1:] if s["packed"])
        side = min(512, W, H)
        rects = {"centre": ((W - side) // 2, (H - side) // 2, side, side), "band": ((W - side) // 2, 0, side, H), "whole": (0, 0, W, H)}
        print(f"# {name}: {W}x{H} K={K} quality {q}, {n_max} containers, {sum(len(b) for b in containers) / n_max / 1e6:.2f} MB each, index "
              f"{sum(len(x) for x in indexes) / n_max / 1e3:.1f} kB each at interval {ia.index_info(indexes[0])['interval']}"
              f"{' (flat band)' if args.flat else ''}", flush=True)
        print(f"# {name}: version-2 index {sum(len(x) for x in indexes2) / n_max / 1e3:.1f} kB each; {packed} of {6 * K} streams packed (frame 0); "
              f"index_extend {extend_ms:.1f} ms a frame, container_index(expanded=True) {build_ms:.1f} ms (frame 0, host)", flush=True)
        out = [torch.empty(3 * W * H, dtype=torch.uint8, device="cuda:0") for _ in range(n_max)]

        def whole_device(n):
            frames, routes = ctx.decode_images_indexed_device(containers[:n], indexes[:n], out=out[:n])
            assert not any(routes), routes
            return frames

        def whole_host(n):
            frames, routes = ctx.decode_images_indexed(containers[:n], indexes[:n])
            assert not any(routes), routes
            return frames

        def region(rect, device, version=1):
            use = indexes2 if version == 2 else indexes

            def run(n):
                if device:
                    frames, routes = ctx.decode_regions_device(containers[:n], use[:n], [rect] * n, out=out[:n])
                else:
                    frames, routes = ctx.decode_regions(containers[:n], use[:n], [rect] * n)
                assert not any(routes), routes
                return frames
            return run
        if args.once:
            n, leg = counts[0], region(rects[args.rect], True, args.index_version)
            leg(n)
            torch.cuda.synchronize()
            t = time.perf_counter()
            leg(n)
            print(f"{name} b{'2' if args.index_version == 2 else ''} {args.rect} n={n}: {(time.perf_counter() - t) * 1e3 / n:.2f} ms/frame", flush=True)
            ctx.close()
            continue
        legs = [("a", whole_device, "decode_images_indexed_device", "a")]
        legs += [(f"b {k}", region(r, True), f"decode_regions_device {r[2]}x{r[3]}", "a") for k, r in rects.items()]
        legs += [(f"b2 {k}", region(r, True, 2), f"decode_regions_device v2 {r[2]}x{r[3]}", f"b {k}") for k, r in rects.items()]
        legs += [("c", whole_host, "decode_images_indexed", "c")]
        legs += [(f"d {k}", region(r, False), f"decode_regions {r[2]}x{r[3]}", "c") for k, r in rects.items()]
        legs += [(f"d2 {k}", region(r, False, 2), f"decode_regions v2 {r[2]}x{r[3]}", f"d {k}") for k, r in rects.items()]
        for n in counts:
            for _, fn, _, _ in legs:                                # warm-up of every shape: buffers grown, pages touched
                fn(n)
            ms = {key: [] for key, _, _, _ in legs}
            for _ in range(args.rounds):
                for key, fn, _, _ in legs:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    res = fn(n)
                    ms[key].append((time.perf_counter() - t) * 1e3 / n)
                    del res
            med = {k: statistics.median(v) for k, v in ms.items()}
            for key, _, label, base in legs:
                v = ms[key]
                print(f"{name} n={n:2d} {key:10s} {label:38s} {med[key]:7.2f} ms/frame (range {min(v):.2f} - {max(v):.2f})  "
                      f"x{med[base] / med[key]:.2f} of {base}", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
