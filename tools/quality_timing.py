#!/usr/bin/env python3
"""quality_timing.py -- mpc_encode_image_quality_device measured, beside what the same question cost before it existed.
    python tools/quality_timing.py [--parent-lib ab_libs/parent/libmpcodec.so] [--out profiles/quality_encode.txt] [--runs 8] [--limit 300]
    python tools/quality_timing.py --leg size:4928x3264:32          (one leg, in this process)
Legs: the three BASELINE sizes (1920x1080 K = 8, 4928x3264 K = 32, 7680x4320 K = 16; quality 3.5; device pixels; frames from bench.py's
generator formula, as tools/budget_timing.py restates it).  Two PSNR targets a size: the full container's PSNR minus 1 dB and minus 3 dB.
Timed, warm-up first, median and range of --runs calls, host clock around calls that return with the container complete, the three
alternated call by call in one process:
    quality   encode_image_quality_device at the target (this library)
    plain     encode_image_device of the same frame (--parent-lib's library: a build of the commit in front of this feature, loaded
              beside this one; without --parent-lib this library, whose code on these paths is the same)
    bisection what a caller had before: a bisection over encode_image_budget_device on the `sse` it reports, to the same target, until
              the bracket of budgets is at most 1/128 of the full container (same library as `plain`); its calls are counted
and alone, with HIP events around it on buffers of its own: the sweep kernel (mpc_budget_sweep_device: the memset of the 768 totals and
the one launch).  Without --leg every leg runs in a fresh child process under its own `timeout`; the first failure stops the script."""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from budget_timing import QUALITY, SIZES, synth_frame                # noqa: E402

DROPS_DB = (1.0, 3.0)


def _span(ms):
    return f"{statistics.median(ms):7.2f} ms ({min(ms):.2f} - {max(ms):.2f})"


def _psnr(sse, W, H):
    return 20.0 * math.log10(765.0) - 10.0 * math.log10(sse / (W * H))


def _second_library(api, path):
    """a context class bound to another build of the library, loaded beside the one already in use"""
    mine, env = api._lib, os.environ.get("MPCODEC_LIB")
    api._lib, os.environ["MPCODEC_LIB"] = None, os.path.abspath(path)
    try:
        other = api.load_library()
    finally:
        api._lib = mine
        if env is None:
            del os.environ["MPCODEC_LIB"]
        else:
            os.environ["MPCODEC_LIB"] = env
    return other


def size_leg(W, H, K, runs, parent_lib):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    from imageexperiments_amd import api
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    before = ctx
    if parent_lib:
        other = _second_library(api, parent_lib)
        mine, api._lib = api._lib, other                             # the context binds the library loaded when it is made
        try:
            before = ia.create_compression_context(K, 8, QUALITY, device=0)
        finally:
            api._lib = mine
        assert before.L is other and ctx.L is not other and not hasattr(other, "mpc_encode_image_quality_device")
    d_rgb = torch.from_numpy(synth_frame(np, W, H, 12345)).cuda()
    tiles = -(-W // 8) * -(-H // 8)
    torch.cuda.synchronize()
    everything = ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, max_sse=(1 << 64) - 1)
    full_psnr = _psnr(everything.full_sse, W, H)
    print(f"{W}x{H} K={K}  full container {everything.full_bytes} bytes, sse {everything.full_sse}, PSNR {full_psnr:.3f} dB; the best a cut reaches: "
          f"sse {everything.min_sse}; `plain` and `bisection` on {'the parent build' if parent_lib else 'this library'}", flush=True)
    # the sweep kernel alone, on buffers of its own
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    d_profile = torch.zeros((tiles, K + 1), dtype=torch.int32, device="cuda")
    d_totals = torch.zeros((256, 3), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, -(-H // 8), d_counts.data_ptr(), d_choices.data_ptr(), stream=stream)
    ctx.depth_profile_device(d_counts.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), W, H, d_profile.data_ptr(), stream=stream)
    weights = ia.budget_weights(ia.container_index(ctx.records_to_container_device(d_counts.data_ptr(), d_choices.data_ptr(), W, H, stream=stream)))
    us = []
    for i in range(12):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        ctx.budget_sweep_device(d_profile.data_ptr(), d_counts.data_ptr(), tiles, weights, d_totals.data_ptr(), stream=stream)
        stop.record()
        stop.synchronize()
        if i >= 2:
            us.append(start.elapsed_time(stop) * 1e3)
    S = d_totals.cpu().numpy().view(np.uint64)
    print(f"  sweep kernel, {tiles} tiles: {statistics.median(us):6.1f} us ({min(us):.1f} - {max(us):.1f}); {len(set(int(v) for v in S[:, 0]))} distinct "
          f"distortion totals along the ladder", flush=True)

    def bisection(max_sse):
        """the smallest budget found whose budget encode reports sse <= max_sse -> (result, calls)"""
        lo, hi, calls, best = 0, everything.full_bytes, 0, None      # lo: too few bytes (or none tried); hi: good enough
        while hi - lo > max(everything.full_bytes // 128, 1):
            mid = (lo + hi) // 2
            calls += 1
            try:
                got = before.encode_image_budget_device(d_rgb.data_ptr(), W, H, mid)
            except ia.MpcError:                                     # below the smallest container there is
                lo = mid
                continue
            if got.sse <= max_sse:
                hi, best = mid, got
            else:
                lo = mid
        return best, calls

    for drop in DROPS_DB:
        target = full_psnr - drop
        max_sse = ia.sse_for_psnr(target, W, H)
        ms = {"quality": [], "plain": [], "bisection": []}
        got = found = None
        calls = 0
        for i in range(2 + runs):
            for what in ms:                                          # alternated call by call
                torch.cuda.synchronize()
                t = time.perf_counter()
                if what == "quality":
                    got = ctx.encode_image_quality_device(d_rgb.data_ptr(), W, H, psnr=target)
                elif what == "plain":
                    before.encode_image_device(d_rgb.data_ptr(), W, H)
                else:
                    found, calls = bisection(max_sse)
                took = (time.perf_counter() - t) * 1e3
                if i >= 2:
                    ms[what].append(took)
        assert got.sse <= max_sse
        print(f"  target PSNR {target:.3f} dB (full - {drop:g}), sse <= {max_sse}: quality encode {_span(ms['quality'])} -> {len(got.container)} bytes at "
              f"multiplier {got.lambda_index}, sse {got.sse}, records {got.records} of {got.full_records}", flush=True)
        print(f"    plain encode {_span(ms['plain'])}   bisection over the budget encode, {calls} calls: {_span(ms['bisection'])} -> "
              f"{'nothing' if found is None else f'{len(found.container)} bytes, sse {found.sse}'}", flush=True)
    if before is not ctx:
        before.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, help="size:WxH:K")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", default=None, help="a build of the commit in front of the target-quality encode")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        _, size, K = args.leg.split(":")
        W, H = size.split("x")
        size_leg(int(W), int(H), int(K), args.runs, args.parent_lib)
        return 0
    lines = [f"# quality {QUALITY}; device pixels; median (range) of {args.runs} calls after 2 warm-up calls, host clock around calls that return with "
             "the container complete, the three kinds alternated call by call; no index asked for"]
    print(lines[0], flush=True)
    status = 0
    for W, H, K in SIZES:
        leg = f"size:{W}x{H}:{K}"
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--runs", str(args.runs)]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += r.stdout.splitlines()
        if r.returncode != 0:                                       # the first failure ends the script: nothing more is started
            sys.stderr.write(r.stderr[-4000:])
            lines.append(f"# {leg} ended with status {r.returncode}; nothing was run after it")
            status = r.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
