#!/usr/bin/env python3
"""delta_encode_timing.py -- a frame sequence in which a fraction of the tiles changes from frame to frame: mpc_delta_encode (device
pixels) against mpc_encode_image_device on the same frames, in the same process and call.
    python tools/delta_encode_timing.py [--out profiles/delta_encode.txt] [--runs 12] [--limit 240]
    python tools/delta_encode_timing.py --leg random:0.1          (one leg, in this process)
Workload: 4928x3264, K = 32, quality 3.5; frames from bench.py's generator formula (restated below), seeds 12345 (A) and 12346 (B).
Every frame of a sequence is A with B's pixels in a set of tiles; from one frame to the next about `fraction` of the tiles swap sides:
    random     a fresh random set of that many tiles swaps
    rectangle  a full-height rectangle of fraction / 2 of the tile columns holds B and jumps by its own width every frame, so the tiles it
               leaves and the tiles it enters change (at 100 % the two halves of the frame alternate)
Fractions 0, 1 %, 10 %, 50 %, 100 %.  Per frame both calls run, alternating, each timed by the host clock around a call that returns with
the container complete; their bytes are compared outside the clock.  mpc_encode_image_device is code the delta encoder does not touch.
Then, over a few frames more, the pursuit's own busy time per call (mpc_kernel_timing_read), and the diff alone -- mp_tile_diff_kernel with
the three small kernels that turn its flags into the list -- from HIP events around mpc_tile_diff_device on buffers of its own.
Without --leg every leg runs in a fresh child process under its own `timeout`; the first failure stops the script, and the collected lines
go to --out."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, K, QUALITY = 4928, 3264, 32, 3.5
FRACTIONS = (0.0, 0.01, 0.1, 0.5, 1.0)
VARIANTS = ("random", "rectangle")


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


def leg(variant, fraction, runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    tx, ty = W // 8, H // 8
    tiles = tx * ty
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    d_a, d_b = (torch.from_numpy(synth_frame(np, W, H, seed)).cuda() for seed in (12345, 12346))
    assert bool((d_a.view(ty, 8, tx, 8, 3) != d_b.view(ty, 8, tx, 8, 3)).any(dim=4).any(dim=3).any(dim=1).all())      # every tile differs
    rng = np.random.default_rng(7)
    side = np.zeros((ty, tx), bool)                                  # True: the tile shows B
    columns = max(int(round(fraction / 2 * tx)), 1)

    def advance(i):
        nonlocal side
        if fraction == 0.0:
            return
        if variant == "random":
            swap = np.zeros(tiles, bool)
            swap[rng.choice(tiles, int(round(fraction * tiles)), replace=False)] = True
            side = side ^ swap.reshape(ty, tx)
        else:
            first = (i % (tx // columns)) * columns              # disjoint places, one after the other; at 100 % the two halves
            side = np.zeros((ty, tx), bool)
            side[:, first:first + columns] = True

    def frame():
        mask = torch.from_numpy(side).cuda().repeat_interleave(8, 0).repeat_interleave(8, 1).unsqueeze(2)
        out = torch.where(mask, d_b, d_a).contiguous()
        torch.cuda.synchronize()
        return out

    enc = ctx.delta_encoder(W, H)
    ms = {"delta": [], "whole": []}
    changed = []
    warm = 3
    for i in range(warm + runs):
        advance(i)
        cur = frame()
        order = ("delta", "whole") if i % 2 == 0 else ("whole", "delta")
        got = {}
        for which in order:
            torch.cuda.synchronize()
            t = time.perf_counter()
            got[which] = enc.encode_device(cur.data_ptr()) if which == "delta" else ctx.encode_image_device(cur.data_ptr(), W, H)
            took = (time.perf_counter() - t) * 1e3
            if i >= warm:
                ms[which].append(took)
        assert got["delta"] == got["whole"], (variant, fraction, i)
        if i >= warm:
            assert enc.info[2] == 0
            changed.append(enc.info[1])
    # the pursuit's share of a call of either kind
    busy = {"delta": [], "whole": []}
    ctx.kernel_timing(True)
    for i in range(warm + runs, warm + runs + 4):
        advance(i)
        cur = frame()
        ctx.read_kernel_timing()
        enc.encode_device(cur.data_ptr())
        busy["delta"].append(ctx.read_kernel_timing()[2])
        ctx.encode_image_device(cur.data_ptr(), W, H)
        busy["whole"].append(ctx.read_kernel_timing()[2])
    ctx.kernel_timing(False)
    # the diff alone: two frames `fraction` apart, alternating, HIP events around the entry point
    advance(warm + runs + 4)
    other = frame()
    kept = cur.clone()
    d_list, d_count = torch.zeros(tiles, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    us = []
    for i in range(24):
        new = other if i % 2 == 0 else cur
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        ctx.tile_diff_device(kept.data_ptr(), new.data_ptr(), W, H, 0, d_list.data_ptr(), d_count.data_ptr(), stream)
        stop.record()
        stop.synchronize()
        if i >= 4:
            us.append(start.elapsed_time(stop) * 1e3)
    md, mw = statistics.median(ms["delta"]), statistics.median(ms["whole"])
    print(f"{variant:9s} {100 * fraction:5.1f} %  changed {statistics.median(changed):8.0f} of {tiles}  "
          f"delta {md:6.2f} ms ({min(ms['delta']):.2f} - {max(ms['delta']):.2f})  whole {mw:6.2f} ms ({min(ms['whole']):.2f} - {max(ms['whole']):.2f})  "
          f"whole / delta {mw / md:5.2f}  pursuit busy {statistics.median(busy['delta']):5.2f} | {statistics.median(busy['whole']):5.2f} ms  "
          f"diff + list {statistics.median(us):6.1f} us ({min(us):.1f} - {max(us):.1f}), {d_count.item()} listed", flush=True)
    enc.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, help="variant:fraction, e.g. random:0.1")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        variant, fraction = args.leg.split(":")
        leg(variant, float(fraction), args.runs)
        return 0
    lines = [f"# {W}x{H} K={K} quality {QUALITY}; per frame, median (range) of {args.runs} frames; delta = mpc_delta_encode (device pixels), "
             "whole = mpc_encode_image_device of the same frame, alternating in one process; pursuit busy: delta | whole"]
    print(lines[0], flush=True)
    status = 0
    for variant in VARIANTS:
        for fraction in FRACTIONS:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", f"{variant}:{fraction}", "--runs",
                   str(args.runs)]
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            lines += r.stdout.splitlines()
            if r.returncode != 0:                                   # the first failure ends the script: nothing more is started
                sys.stderr.write(r.stderr[-4000:])
                lines.append(f"# {variant}:{fraction} ended with status {r.returncode}; nothing was run after it")
                status = r.returncode
                break
        if status:
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
