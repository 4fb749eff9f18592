#!/usr/bin/env python3
"""index_scan_timing.py -- the seek index from a device bit scan against the serial parse, in one process.
    python tools/index_scan_timing.py [--workloads raise,1080p,mn] [--frames 1,16] [--rounds 5] [--once]
For n distinct containers of a workload (bench.py's: synthetic frames, seeds 12345 + f, encoded untimed here; `mn`: the golden
.mn of the reference, n copies of it):
    a  ia.container_index               the host's serial build of the index (one frame)
    b  ctx.container_index_device       the same blob from the device scan (one frame)
    c  ctx.decode_images_device         frames without an index by the serial route
    d  ctx.decode_images_scan_device    frames without an index: device scan, then the indexed route
    e  ctx.decode_images_indexed_device with prebuilt indexes: the floor of d
Output buffers are allocated before the clock.  After a warm-up of every leg the legs alternate, `rounds` times; host clock around
calls that return with their result complete.  Prints median and range of ms (a, b: per container; c - e: per call and per frame).
--once: a warm-up and one call of leg d on one frame of the first workload, nothing else (for MPC_TRACE=1: the scan's share)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="raise,1080p,mn")
    ap.add_argument("--frames", default="1,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    import imageexperiments_amd as ia
    from bench import WORKLOADS, synth_frame
    counts = [int(v) for v in args.frames.split(",")]
    n_max = max(counts)
    for name in args.workloads.split(","):
        if name == "mn":
            with open(os.path.join(ROOT, "tests", "golden", "r0c1de5e1t_3_5.mn"), "rb") as f:
                mn = f.read()
            W, H, K, _ = ia.container_info(mn)
            ctx = ia.create_compression_context(K, 8, 3.5, device=0)
            containers = [mn] * n_max
        else:
            W, H, K, q = WORKLOADS[name]
            ctx = ia.create_compression_context(K, 8, q, device=0)
            containers = []
            for lo in range(0, n_max, 8):                          # encoded eight at a time: the frames' host memory
                containers += [bytes(b) for b in ctx.encode_images([synth_frame(W, H, 12345 + f) for f in range(lo, min(n_max, lo + 8))])]
        indexes = [ia.container_index(b) for b in containers]
        out = [torch.empty(3 * W * H, dtype=torch.uint8, device="cuda:0") for _ in range(n_max)]
        print(f"# {name}: {W}x{H} K={K}, {n_max} containers, {sum(len(b) for b in containers) / n_max / 1e6:.2f} MB each, index "
              f"{len(indexes[0]) / 1e3:.1f} kB at interval {ia.index_info(indexes[0])['interval']}", flush=True)

        def host_build(n):
            assert ia.container_index(containers[0]) == indexes[0]

        def device_build(n):
            blob, route = ctx.container_index_device(containers[0])
            assert route == 0 and blob == indexes[0]

        def serial(n):
            ctx.decode_images_device(containers[:n], out=out[:n])

        def scan(n):
            _, routes = ctx.decode_images_scan_device(containers[:n], out=out[:n])
            assert not any(routes), routes

        def indexed(n):
            _, routes = ctx.decode_images_indexed_device(containers[:n], indexes[:n], out=out[:n])
            assert not any(routes), routes

        if args.once:
            scan(1)
            print("# the traced call follows", file=sys.stderr, flush=True)
            scan(1)
            ctx.close()
            return
        legs = [("a container_index (host)", host_build, [1]), ("b container_index_device", device_build, [1]),
                ("c decode_images_device", serial, counts), ("d decode_images_scan_device", scan, counts),
                ("e decode_images_indexed_device", indexed, counts)]
        times = {}
        for _, call, ns in legs:
            for n in ns:
                call(n)                                             # warm-up: buffers grown, tables resident
        for _ in range(args.rounds):
            for label, call, ns in legs:
                for n in ns:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    call(n)
                    torch.cuda.synchronize()
                    times.setdefault((label, n), []).append((time.perf_counter() - t) * 1e3)
        for (label, n), ms in times.items():
            print(f"{name:6s} {label:32s} n={n:2d}  median {statistics.median(ms):8.2f} ms a call ({statistics.median(ms) / n:7.2f} a frame)  "
                  f"range {min(ms):8.2f} .. {max(ms):8.2f}", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
