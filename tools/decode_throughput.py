#!/usr/bin/env python3
"""decode_throughput.py -- decoding n containers in one call against n single-frame calls (one decoder behind both), in one process.
    python tools/decode_throughput.py [--workloads raise,1080p] [--frames 1,4,16,32] [--rounds 5] [--interval 0,...] [--once]
For n distinct containers of a workload (bench.py's: synthetic frames, seeds 12345 + f, encoded untimed here):
    a  a loop of decode_image          (mpc_decode_image: one frame a call, host pixels; the baseline)
    b  decode_images                   (mpc_decode_images: host pixels)
    c  decode_images_device            (mpc_decode_images_device: pixels left in device memory, buffers allocated before the clock)
    d  decode_images_indexed           (mpc_decode_images_indexed: b with a seek index per frame, the entropy codes parsed on the device)
    e  decode_images_indexed_device    (mpc_decode_images_indexed_device: c with a seek index per frame)
The indexes are built before the clock (container_index at --interval, 0 = the library's default; several values: the whole
table once per value); their build time and size are reported.  After a warm-up of every shape the five alternate, `rounds`
times; host clock around calls that return with the pixels complete.  Prints median and range of ms per frame, Mpix/s of the
median, and each against a.  b and c are the serial routes: the baselines of d and e in the same run.
--once: a warm-up and one pass of one leg (--leg c or e, default e) over 16 frames, nothing else (for a kernel trace or
MPC_TRACE=1)."""
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
    ap.add_argument("--frames", default="1,4,16,32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--interval", default="0")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--leg", default="e", choices=["c", "e"])
    args = ap.parse_args()
    import torch
    import imageexperiments_amd as ia
    from bench import WORKLOADS, synth_frame
    counts = [int(v) for v in args.frames.split(",")]
    for name in args.workloads.split(","):
        W, H, K, q = WORKLOADS[name]
        ctx = ia.create_compression_context(K, 8, q, device=0)
        n_max = 16 if args.once else max(counts)
        containers = []
        for lo in range(0, n_max, 8):                              # encoded eight at a time: 8 x 48 MB of frames in host memory
            containers += ctx.encode_images([synth_frame(W, H, 12345 + f) for f in range(lo, min(n_max, lo + 8))])
        mpix = W * H / 1e6
        print(f"# {name}: {W}x{H} K={K} quality {q}, {n_max} containers, {sum(len(b) for b in containers) / n_max / 1e6:.2f} MB each",
              flush=True)
        out = [torch.empty(3 * W * H, dtype=torch.uint8, device="cuda:0") for _ in range(n_max)]

        def a(n):
            return [ia.decode_image(b, ctx) for b in containers[:n]]

        def b(n):
            return ctx.decode_images(containers[:n])

        def c(n):
            return ctx.decode_images_device(containers[:n], out=out[:n])
        for interval in [int(v) for v in args.interval.split(",")]:
            t = time.perf_counter()
            indexes = [ia.container_index(blob, interval) for blob in containers]
            build_ms = (time.perf_counter() - t) * 1e3 / n_max
            print(f"# {name} interval {ia.index_info(indexes[0])['interval']}: index {sum(len(x) for x in indexes) / n_max / 1e3:.1f} kB a frame, "
                  f"built in {build_ms:.1f} ms a frame on one host thread", flush=True)

            def d(n):
                frames, routes = ctx.decode_images_indexed(containers[:n], indexes[:n])
                assert not any(routes), routes
                return frames

            def e(n):
                frames, routes = ctx.decode_images_indexed_device(containers[:n], indexes[:n], out=out[:n])
                assert not any(routes), routes
                return frames
            if args.once:
                leg = c if args.leg == "c" else e
                leg(16)
                torch.cuda.synchronize()
                t = time.perf_counter()
                leg(16)
                print(f"{name} {args.leg} n=16: {(time.perf_counter() - t) * 1e3 / 16:.2f} ms/frame", flush=True)
                continue
            legs = (("a", a, "decode_image loop"), ("b", b, "decode_images"), ("c", c, "decode_images_device"),
                    ("d", d, "decode_images_indexed"), ("e", e, "decode_images_indexed_device"))
            for n in counts:
                for _, fn, _ in legs:                               # warm-up of every shape: buffers grown, pages touched
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
                    print(f"{name} n={n:2d} {key} {label:28s} {med[key]:7.2f} ms/frame (range {min(v):.2f} - {max(v):.2f})  "
                          f"{mpix / med[key] * 1e3:7.0f} Mpix/s  x{med['a'] / med[key]:.2f} of a", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
