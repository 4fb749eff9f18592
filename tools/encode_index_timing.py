#!/usr/bin/env python3
"""encode_index_timing.py -- what a seek index costs at encode time, against building it from the finished container.
    python tools/encode_index_timing.py [--workloads raise,1080p] [--frames 16] [--rounds 5] [--interval 128] [--legs a,b,c]
For n frames of a workload (bench.py's: synthetic frames, seeds 12345 + f) resident in device memory:
    a  encode_images_device                      (mpc_encode_images_device: the containers alone)
    b  encode_images_indexed_device              (mpc_encode_images_indexed_device: containers and indexes from the entropy stage)
    c  a, then container_index on every container (mpc_container_index: one serial parse per container on one host thread)
    d  encode_images_indexed_device(expanded=True) (mpc_encode_images_indexed2_device: index version 2, the aux entries from the
       entropy stage as well)
    e  b, then index_extend on every container   (mpc_index_extend: the aux entries on one host thread, a chunked parse and a linear pass)
The profiler is off.  Every shape is warmed up, then the legs alternate `rounds` times; host clock around calls that return with
their results complete.  Prints median and range of ms per frame per leg, and the figure of merit: (b) - (a) against (c) - (a).
b and c are checked once to give the same indexes, d and e to give the same version-2 indexes; with both, the second figure of
merit: what the aux section costs at encode time, (d) - (b), against what it costs on the host, (e) - (b).
--legs a (or a,b): what a library without the indexed (or the ...indexed2) entry points can run (MPCODEC_LIB=<an older build>): its
medians on the same box in the same call are what this build's are compared with.
--once: a warm-up and one pass of leg b, nothing else (for a kernel trace)."""
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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--interval", type=int, default=128)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    from bench import WORKLOADS, synth_frame
    n = args.frames
    wanted = args.legs.split(",")
    print(f"# library {ia.library_path()}", flush=True)
    for name in args.workloads.split(","):
        W, H, K, q = WORKLOADS[name]
        ctx = ia.create_compression_context(K, 8, q, device=0)
        d_frames = [torch.from_numpy(np.ascontiguousarray(synth_frame(W, H, 12345 + f))).cuda() for f in range(n)]
        ptrs = [t.data_ptr() for t in d_frames]

        def a():
            return ctx.encode_images_device(ptrs, W, H)

        def b():
            return ctx.encode_images_indexed_device(ptrs, W, H, args.interval)

        def c():
            return [(blob, ia.container_index(blob, args.interval)) for blob in ctx.encode_images_device(ptrs, W, H)]

        def d():
            return ctx.encode_images_indexed_device(ptrs, W, H, args.interval, expanded=True)

        def e():
            return [(blob, ia.index_extend(blob, index)) for blob, index in b()]
        legs = [leg for leg in (("a", a, "encode_images_device"), ("b", b, "encode_images_indexed_device"),
                                ("c", c, "encode_images_device + container_index"),
                                ("d", d, "encode_images_indexed_device(expanded)"),
                                ("e", e, "encode_images_indexed_device + index_extend")) if leg[0] in wanted]
        if args.once:
            b()
            torch.cuda.synchronize()
            t = time.perf_counter()
            b()
            print(f"{name} b n={n}: {(time.perf_counter() - t) * 1e3 / n:.2f} ms/frame", flush=True)
            ctx.close()
            continue
        results = {key: fn() for key, fn, _ in legs}                # warm-up of every shape: buffers grown, pages touched
        if "b" in results and "c" in results:
            assert results["b"] == results["c"], "the encoder's indexes differ from container_index's"
            print(f"# {name}: {W}x{H} K={K} quality {q}, {n} frames, {sum(len(x) for x, _ in results['b']) / n / 1e6:.2f} MB a container, "
                  f"{sum(len(x) for _, x in results['b']) / n / 1e3:.1f} kB an index (interval {args.interval})", flush=True)
        if "d" in results and "e" in results:
            assert results["d"] == results["e"], "the encoder's version-2 indexes differ from index_extend's"
            print(f"# {name}: {sum(len(x) for _, x in results['d']) / n / 1e3:.1f} kB a version-2 index", flush=True)
        del results
        ms = {key: [] for key, _, _ in legs}
        for _ in range(args.rounds):
            for key, fn, _ in legs:
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = fn()
                ms[key].append((time.perf_counter() - t) * 1e3 / n)
                del res
        med = {k: statistics.median(v) for k, v in ms.items()}
        for key, _, label in legs:
            v = ms[key]
            print(f"{name} n={n} {key} {label:40s} {med[key]:7.3f} ms/frame (range {min(v):.3f} - {max(v):.3f})  "
                  f"{W * H / 1e6 / med[key] * 1e3:7.0f} Mpix/s", flush=True)
        if all(k in med for k in "abc"):
            spread = max(ms["a"]) - min(ms["a"])
            print(f"{name} n={n} index at encode time (b - a) {med['b'] - med['a']:+.3f} ms/frame; from the container (c - a) "
                  f"{med['c'] - med['a']:+.3f} ms/frame; spread of a {spread:.3f} ms/frame", flush=True)
        if all(k in med for k in "bde"):
            spread = max(ms["b"]) - min(ms["b"])
            print(f"{name} n={n} aux at encode time (d - b) {med['d'] - med['b']:+.3f} ms/frame; on the host (e - b) "
                  f"{med['e'] - med['b']:+.3f} ms/frame; spread of b {spread:.3f} ms/frame", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
