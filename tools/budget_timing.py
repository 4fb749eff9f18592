#!/usr/bin/env python3
"""budget_timing.py -- mpc_encode_image_budget_device measured: what a container of a given size costs, and what the per-tile cut buys.
    python tools/budget_timing.py [--out profiles/budget_encode.txt] [--runs 8] [--limit 300]
    python tools/budget_timing.py --leg size:4928x3264:32          (one leg, in this process)
    python tools/budget_timing.py --leg photo
Legs `size`: the three BASELINE sizes (1920x1080 K = 8, 4928x3264 K = 32, 7680x4320 K = 16; quality 3.5; frames from bench.py's generator
formula, restated below).  For budgets of 1/2 and 1/4 of the full container: ms per call of the budget encode (host clock around a call
that returns with the container complete), its probes, and -- from the public pieces on buffers of their own -- the profile kernel alone
(HIP events around mpc_depth_profile_device) and one probe (allocation kernel + records -> container, host clock); beside them
mpc_encode_image_device of the same frame and mpc_rate_distortion_device over as many quality levels as the budget encode made
containers, which is what a caller had before.
Leg `photo`: the reference's photograph (tests/golden, decoded by the product), K = 32: for m = 1, 2, 4, 8 the uniform cut
mpc_truncate_container(F, m), its size B and squared error, against the budget encode at B.  Reported, not asserted: the rate model is
an average per stream.
Without --leg every leg runs in a fresh child process under its own `timeout`; the first failure stops the script, and the collected
lines go to --out."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUALITY = 3.5
SIZES = ((1920, 1080, 8), (4928, 3264, 32), (7680, 4320, 16))
FRACTIONS = (2, 4)


def synth_frame(np, width, height, seed):
    """bench.py's generator, restated: std::mt19937(seed), raster order, one draw per pixel; n = draw % 32 - 16;
    (R, G, B) = clip(x * 255 / W + n), clip(y * 255 / H + n), clip(128 + 3 n)"""
    bg = np.random.MT19937()
    state = bg.state
    key = np.empty(624, np.uint32)
    key[0] = seed & 0xFFFFFFFF
    for i in range(1, 624):
        key[i] = (1812433253 * (int(key[i - 1]) ^ (int(key[i - 1]) >> 30)) + i) & 0xFFFFFFFF
    state["state"]["key"] = key
    state["state"]["pos"] = 624
    bg.state = state
    n = bg.random_raw(width * height).astype(np.int64).reshape(height, width) % 32 - 16
    x = np.arange(width, dtype=np.int64)[None, :]
    y = np.arange(height, dtype=np.int64)[:, None]
    out = np.empty((height, width, 3), np.uint8)
    out[..., 0] = np.clip(x * 255 // width + n, 0, 255)
    out[..., 1] = np.clip(y * 255 // height + n, 0, 255)
    out[..., 2] = np.clip(128 + 3 * n, 0, 255)
    return out


def _clock(torch, call, runs, warm=2):
    ms, out = [], None
    for i in range(warm + runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        took = (time.perf_counter() - t) * 1e3
        if i >= warm:
            ms.append(took)
    return ms, out


def _span(ms):
    return f"{statistics.median(ms):7.2f} ms ({min(ms):.2f} - {max(ms):.2f})"


def size_leg(W, H, K, runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    d_rgb = torch.from_numpy(synth_frame(np, W, H, 12345)).cuda()
    tiles = -(-W // 8) * -(-H // 8)
    whole_ms, full = _clock(torch, lambda: ctx.encode_image_device(d_rgb.data_ptr(), W, H), runs)
    print(f"{W}x{H} K={K}  full container {len(full)} bytes  encode_image_device {_span(whole_ms)}", flush=True)
    # the public pieces on buffers of their own
    d_counts = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_choices = torch.zeros((tiles, 3, K), dtype=torch.int32, device="cuda")
    d_profile = torch.zeros((tiles, K + 1), dtype=torch.int32, device="cuda")
    d_depth = torch.zeros(tiles, dtype=torch.uint8, device="cuda")
    d_cut = torch.zeros((tiles, 3), dtype=torch.int16, device="cuda")
    d_totals = torch.zeros(3, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.encode_tiles_device(d_rgb.data_ptr(), W, H, 3 * W, 0, -(-H // 8), d_counts.data_ptr(), d_choices.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    us = []
    for i in range(12):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        ctx.depth_profile_device(d_counts.data_ptr(), d_choices.data_ptr(), d_rgb.data_ptr(), W, H, d_profile.data_ptr(), stream=stream, check=False)
        stop.record()
        stop.synchronize()
        if i >= 2:
            us.append(start.elapsed_time(stop) * 1e3)
    weights = ia.budget_weights(ia.container_index(full))
    for k in FRACTIONS:
        budget = len(full) // k
        ms, got = _clock(torch, lambda: ctx.encode_image_budget_device(d_rgb.data_ptr(), W, H, budget), runs)
        assert len(got.container) <= budget

        def probe():
            ctx.budget_allocate_device(d_profile.data_ptr(), d_counts.data_ptr(), tiles, weights, got.lambda_index, d_depth.data_ptr(),
                                       d_cut.data_ptr(), d_totals.data_ptr(), stream=stream)
            return ctx.records_to_container_device(d_cut.data_ptr(), d_choices.data_ptr(), W, H, stream=stream)
        probe_ms, blob = _clock(torch, probe, runs)
        assert blob == got.container
        levels = [8.0 - 6.0 * i / got.probes for i in range(got.probes + 1)]         # as many containers as the budget encode made
        sweep_ms, points = _clock(torch, lambda: ctx.rate_distortion_device(d_rgb.data_ptr(), W, H, levels), max(runs // 2, 2), warm=1)
        nearest = min((p for p in points), key=lambda p: abs(p.size - budget))
        print(f"  budget 1/{k} = {budget} bytes: {len(got.container)} bytes at multiplier {got.lambda_index}, {got.probes} probes  "
              f"budget encode {_span(ms)}  profile kernel {statistics.median(us):6.1f} us ({min(us):.1f} - {max(us):.1f})  "
              f"one probe {_span(probe_ms)}  records {got.records} of {got.full_records}  sse {got.sse} (full {got.full_sse})", flush=True)
        print(f"    rate_distortion_device, {len(levels)} levels: {_span(sweep_ms)}; its level nearest the budget: {nearest.size} bytes, sse {nearest.sse}",
              flush=True)
    ctx.close()


def photo_leg():
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    K = 32
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    with open(os.path.join(ROOT, "tests", "golden", "r0c1de5e1t_3_5.mn"), "rb") as f:
        rgb = np.ascontiguousarray(ia.decode_image(f.read(), ctx))
    H, W = rgb.shape[:2]
    full = ctx.encode_image(rgb)
    d_rgb = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    print(f"photograph {W}x{H} K={K}: full container {len(full)} bytes", flush=True)
    for m in (1, 2, 4, 8):
        cut = ia.truncate_container(full, m)
        decoded = np.asarray(ia.decode_image(cut, ctx))
        sse_cut = int(((decoded.astype(np.int64) - rgb.astype(np.int64)) ** 2).sum())
        got = ctx.encode_image_budget_device(d_rgb.data_ptr(), W, H, len(cut))
        print(f"  m = {m}: uniform cut {len(cut)} bytes, sse {sse_cut}   budget encode {len(got.container)} bytes, sse {got.sse} "
              f"({got.sse / sse_cut:.3f} of the uniform cut's), multiplier {got.lambda_index}, {got.probes} probes, depth mean {got.depth.mean():.2f} "
              f"max {int(got.depth.max())}", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, help="size:WxH:K or photo")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--limit", type=int, default=300, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        if args.leg == "photo":
            photo_leg()
        else:
            _, size, K = args.leg.split(":")
            W, H = size.split("x")
            size_leg(int(W), int(H), int(K), args.runs)
        return 0
    lines = [f"# quality {QUALITY}; median (range) of {args.runs} calls, host clock around calls that return with the container complete; "
             "budget encode = mpc_encode_image_budget_device, no index asked for"]
    print(lines[0], flush=True)
    status = 0
    for leg in [f"size:{W}x{H}:{K}" for W, H, K in SIZES] + ["photo"]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--runs", str(args.runs)]
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
