#!/usr/bin/env python3
"""decode_view_timing.py -- views of a frame (its first steps, reduced 2/4/8x) through its seek index against the whole decode, in
one process.
    python tools/decode_view_timing.py [--workloads raise,1080p] [--frames 1,16] [--rounds 5] [--interval 0] [--index-version 2]
                                       [--once LEG]
For n distinct containers of a workload (bench.py's: synthetic frames, seeds 12345 + f, encoded with their indexes untimed here):
    a        decode_images_indexed_device            the whole frame, pixels left in device memory: the baseline of b - e
    a host   decode_images_indexed                   the same with host pixels: the baseline of e host
    b        decode_views_device, steps 0, scale 0   the whole frame as a view: what the windowed route costs over a
    c m      ... steps m in 1, 2, 4, scale 0         the streams of steps >= m are never read
    d s      ... steps 0, scale_log2 s in 1, 2, 3    1/4, 1/16, 1/64 of the pixels leave the reconstruction kernel
    e        ... steps 1, scale_log2 3               a thumbnail; e host: decode_views, the thumbnail in host memory
Every leg takes the same index (--index-version; 2 = index_extend of the encoder's index, made before the clock).  Also printed: the
container cut to 1, 2 and 4 steps by truncate_container against its whole size.  Output buffers are allocated before the clock.
After a warm-up of every shape the legs alternate, `rounds` times; host clock around calls that return with the pixels complete.
Prints median and range of ms per frame and each against its baseline.
--once LEG: a warm-up and one pass of that leg (a, b, e, ...) over n frames of the first --frames value, nothing else (for a
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
    ap.add_argument("--workloads", default="raise,1080p")
    ap.add_argument("--frames", default="1,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--interval", type=int, default=0)
    ap.add_argument("--index-version", type=int, default=2, choices=[1, 2])
    ap.add_argument("--once", default=None)
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
        for lo in range(0, n_max, 8):                              # encoded eight at a time: 8 x 48 MB of frames in host memory
            pairs += ctx.encode_images_indexed([synth_frame(W, H, 12345 + f) for f in range(lo, min(n_max, lo + 8))], args.interval)
        containers, indexes = [p[0] for p in pairs], [p[1] for p in pairs]
        if args.index_version == 2:
            indexes = [ia.index_extend(b, x) for b, x in zip(containers, indexes)]
        cut = {m: len(ia.truncate_container(containers[0], m)) for m in (1, 2, 4)}
        print(f"# {name}: {W}x{H} K={K} quality {q}, {n_max} containers, {sum(len(b) for b in containers) / n_max / 1e6:.2f} MB each, version-"
              f"{args.index_version} index {sum(len(x) for x in indexes) / n_max / 1e3:.1f} kB each at interval "
              f"{ia.index_info(indexes[0])['interval']}", flush=True)
        print(f"# {name}: frame 0 is {len(containers[0])} bytes; cut to 1, 2, 4 steps {cut[1]}, {cut[2]}, {cut[4]} bytes", flush=True)
        out = [torch.empty(3 * W * H, dtype=torch.uint8, device="cuda:0") for _ in range(n_max)]

        def whole_device(n):
            frames, routes = ctx.decode_images_indexed_device(containers[:n], indexes[:n], out=out[:n])
            assert not any(routes), routes
            return frames

        def whole_host(n):
            frames, routes = ctx.decode_images_indexed(containers[:n], indexes[:n])
            assert not any(routes), routes
            return frames

        def view(steps, scale_log2, device=True):
            def run(n):
                views = [(None, steps, scale_log2)] * n
                if device:
                    frames, routes = ctx.decode_views_device(containers[:n], indexes[:n], views, out=out[:n])
                else:
                    frames, routes = ctx.decode_views(containers[:n], indexes[:n], views)
                assert not any(routes), routes
                return frames
            return run
        legs = [("a", whole_device, "decode_images_indexed_device", "a"), ("a host", whole_host, "decode_images_indexed", "a host"),
                ("b", view(0, 0), "decode_views_device steps 0 scale 0", "a")]
        legs += [(f"c {m}", view(m, 0), f"decode_views_device steps {m} scale 0", "a") for m in (1, 2, 4)]
        legs += [(f"d {s}", view(0, s), f"decode_views_device steps 0 scale {s}", "a") for s in (1, 2, 3)]
        legs += [("e", view(1, 3), "decode_views_device steps 1 scale 3", "a"), ("e host", view(1, 3, False), "decode_views steps 1 scale 3", "a host")]
        if args.once:
            n, leg = counts[0], {key: fn for key, fn, _, _ in legs}[args.once]
            leg(n)
            torch.cuda.synchronize()
            t = time.perf_counter()
            leg(n)
            print(f"{name} {args.once} n={n}: {(time.perf_counter() - t) * 1e3 / n:.2f} ms/frame", flush=True)
            ctx.close()
            continue
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
                print(f"{name} n={n:2d} {key:7s} {label:38s} {med[key]:7.2f} ms/frame (range {min(v):.2f} - {max(v):.2f})  "
                      f"x{med[base] / med[key]:.2f} of {base}", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
