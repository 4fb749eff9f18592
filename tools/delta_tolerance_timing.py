#!/usr/bin/env python3
"""delta_tolerance_timing.py -- what the delta encoder's change tolerance costs and what it buys.
    python tools/delta_tolerance_timing.py [--out profiles/delta_tolerance.txt] [--runs 12] [--limit 300] [--parent-lib OLD.so]
    python tools/delta_tolerance_timing.py --leg kernel          (one leg, in this process)
Workload: 4928x3264, K = 32, quality 3.5, device pixels.  Three legs, each in a fresh child process under its own `timeout`; the first
failure stops the script, and the collected lines go to --out.
  kernel   mp_tile_diff_tol_kernel against mp_tile_diff_kernel (each with the three flags -> list kernels), HIP events around
           mpc_tile_diff_tolerance_device and mpc_tile_diff_device on kept copies of their own, alternating call by call in one process,
           the new frame alternating between two: bench.py's frames A and B mixed so that 1 % of the tiles differ (every other tile byte
           for byte equal), and the noisy natural sequence below.  Median of 20 behind 4 warm-up calls.
  session  mpc_delta_encode on the 1 % random case of profiles/delta_encode.txt (tools/delta_encode_timing.py's frames), a session at
           tolerance 0.  With --parent-lib the same leg runs with that build of the library (MPCODEC_LIB) and with this one, three
           times each, alternating: the parent's own run-to-run range is what this one has to fall into.
  noise    the case the tolerance exists for: the natural photo of tests/golden plus fresh Gaussian noise of sigma 2 in every frame,
           plus a rectangle of 1 % of the tiles that moves by its own width.  For tolerance 0 and a few tolerances round the noise's
           expected tile sum (192 * 2 * sigma^2 = 1536 between two noisy frames): the share of tiles changed, ms per mpc_delta_encode
           and per mpc_delta_encode_patch (sessions of their own, alternating on the same frames), patch bytes, and the composite's
           PSNR against the frame from mpc_delta_held."""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.delta_encode_timing import H, K, QUALITY, W, synth_frame  # noqa: E402

TOLERANCES = (0, 1000, 1536, 2500, 4000)
SIGMA = 2.0


def natural(np):
    from PIL import Image
    rgb = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "r0c1de5e1t.jpg")).convert("RGB"), np.uint8)
    assert rgb.shape == (H, W, 3), rgb.shape
    return rgb


def noisy_frames(np, torch, n):
    """the photo under fresh noise, a bright rectangle of 1 % of the tiles moving by its own width -> device frames"""
    tx, ty = W // 8, H // 8
    base = torch.from_numpy(natural(np)).cuda().to(torch.int16)
    gen = torch.Generator(device="cuda").manual_seed(7)
    cols, rows = tx // 10, ty // 10                                  # 61 x 40 tiles: 0.97 % of 251328
    out = []
    for i in range(n):
        px = base + torch.round(torch.randn(base.shape, generator=gen, device="cuda") * SIGMA).to(torch.int16)
        x0, y0 = 8 * ((i * cols) % (tx - cols)), 8 * (ty // 3)
        px[y0:y0 + 8 * rows, x0:x0 + 8 * cols] += 40
        out.append(px.clamp_(0, 255).to(torch.uint8).contiguous())
    torch.cuda.synchronize()
    return out


def swapped_frames(np, torch, n, fraction=0.01):
    """tools/delta_encode_timing.py's random case: A with B's pixels in a set of tiles, `fraction` of the tiles swapping every frame"""
    tx, ty = W // 8, H // 8
    d_a, d_b = (torch.from_numpy(synth_frame(np, W, H, seed)).cuda() for seed in (12345, 12346))
    rng = np.random.default_rng(7)
    side = np.zeros((ty, tx), bool)
    out = []
    for _ in range(n):
        swap = np.zeros(tx * ty, bool)
        swap[rng.choice(tx * ty, int(round(fraction * tx * ty)), replace=False)] = True
        side = side ^ swap.reshape(ty, tx)
        mask = torch.from_numpy(side).cuda().repeat_interleave(8, 0).repeat_interleave(8, 1).unsqueeze(2)
        out.append(torch.where(mask, d_b, d_a).contiguous())
    torch.cuda.synchronize()
    return out


def leg_kernel():
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    tiles = (W // 8) * (H // 8)
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    d_list, d_count = torch.zeros(tiles, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    d_sse = torch.zeros(tiles, dtype=torch.int32, device="cuda")
    for name, frames, tolerance in (("1 % of the tiles swapped", swapped_frames(np, torch, 2), 1000), ("photo + noise, sigma 2", noisy_frames(np, torch, 2), 2500)):
        kept = {"old": frames[1].clone(), "new": frames[1].clone(), "new+sse": frames[1].clone()}
        us = {k: [] for k in kept}
        listed = {}
        for i in range(24):
            cur = frames[i % 2]
            for which in (("old", "new", "new+sse") if i % 2 == 0 else ("new+sse", "new", "old")):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                if which == "old":
                    ctx.tile_diff_device(kept[which].data_ptr(), cur.data_ptr(), W, H, 0, d_list.data_ptr(), d_count.data_ptr(), stream)
                else:
                    ctx.tile_diff_tolerance_device(kept[which].data_ptr(), cur.data_ptr(), W, H, 0, tolerance, d_list.data_ptr(), d_count.data_ptr(),
                                                   d_sse.data_ptr() if which == "new+sse" else 0, stream)
                stop.record()
                stop.synchronize()
                listed[which] = d_count.item()
                if i >= 4:
                    us[which].append(start.elapsed_time(stop) * 1e3)
        text = "  ".join(f"{k} {statistics.median(v):6.1f} us ({min(v):.1f} - {max(v):.1f}), {listed[k]} listed" for k, v in us.items())
        print(f"kernel   {name:26s} T {tolerance:5d}  diff + list: {text}", flush=True)
    ctx.close()


def leg_session(runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    warm = 3
    frames = swapped_frames(np, torch, warm + runs)
    enc = ctx.delta_encoder(W, H)
    if hasattr(enc.L, "mpc_delta_set_tolerance"):
        enc.set_tolerance(0)
    ms, changed = [], []
    for i, cur in enumerate(frames):
        torch.cuda.synchronize()
        t = time.perf_counter()
        enc.encode_device(cur.data_ptr())
        took = (time.perf_counter() - t) * 1e3
        if i >= warm:
            ms.append(took)
            changed.append(enc.info[1])
    print(f"session  {os.path.basename(os.path.dirname(ia.library_path())) or 'lib'}/{os.path.basename(ia.library_path())}  random 1 %  "
          f"changed {statistics.median(changed):6.0f}  mpc_delta_encode {statistics.median(ms):6.2f} ms ({min(ms):.2f} - {max(ms):.2f})", flush=True)
    enc.close()
    ctx.close()


def leg_noise(runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    tiles = (W // 8) * (H // 8)
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    warm = 2
    frames = noisy_frames(np, torch, warm + runs)
    for tolerance in TOLERANCES:
        enc, pat = ctx.delta_encoder(W, H), ctx.delta_encoder(W, H)
        enc.set_tolerance(tolerance)
        pat.set_tolerance(tolerance)
        ms = {"encode": [], "patch": []}
        changed, nbytes, pbytes, psnr = [], [], [], []
        for i, cur in enumerate(frames):
            for which in (("encode", "patch") if i % 2 == 0 else ("patch", "encode")):
                torch.cuda.synchronize()
                t = time.perf_counter()
                blob = enc.encode_device(cur.data_ptr()) if which == "encode" else pat.encode_patch_device(cur.data_ptr(), index_interval=0)
                took = (time.perf_counter() - t) * 1e3
                if i >= warm:
                    ms[which].append(took)
                    (nbytes if which == "encode" else pbytes).append(len(blob))
            assert enc.info[:2] == pat.info[:2] and enc.held() == pat.held()       # a patch of every tile calls itself a key patch
            if i >= warm:
                assert enc.info[2] == 0
                changed.append(enc.info[1])
                mse = enc.held()[1] / (3.0 * W * H)
                psnr.append(10 * math.log10(255.0 ** 2 / mse) if mse > 0 else float("inf"))
        print(f"noise    T {tolerance:5d}  changed {100 * statistics.median(changed) / tiles:6.2f} %  "
              f"mpc_delta_encode {statistics.median(ms['encode']):6.2f} ms ({min(ms['encode']):.2f} - {max(ms['encode']):.2f})  "
              f"mpc_delta_encode_patch {statistics.median(ms['patch']):6.2f} ms ({min(ms['patch']):.2f} - {max(ms['patch']):.2f})  "
              f"container {statistics.median(nbytes):9.0f} B  patch {statistics.median(pbytes):9.0f} B  composite PSNR {statistics.median(psnr):6.2f} dB", flush=True)
        enc.close()
        pat.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=("kernel", "session", "noise"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=300, help="seconds a leg's process may take")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's build of the library, for the session leg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        {"kernel": leg_kernel, "session": lambda: leg_session(args.runs), "noise": lambda: leg_noise(args.runs)}[args.leg]()
        return 0
    lines = [f"# {W}x{H} K={K} quality {QUALITY}, device pixels; median (range); sessions: per frame over {args.runs} frames behind the warm-up"]
    print(lines[0], flush=True)
    legs = [("kernel", None)]
    if args.parent_lib:
        legs += [("session", lib) for _ in range(3) for lib in (os.path.abspath(args.parent_lib), None)]
    else:
        legs += [("session", None)]
    legs += [("noise", None)]
    status = 0
    for name, lib in legs:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--runs", str(args.runs)]
        env = dict(os.environ)
        env.pop("MPCODEC_LIB", None)
        if lib:
            env["MPCODEC_LIB"] = lib
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=env)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += r.stdout.splitlines()
        if r.returncode != 0:                                       # the first failure ends the script: nothing more is started
            sys.stderr.write(r.stderr[-4000:])
            lines.append(f"# {name} ended with status {r.returncode}; nothing was run after it")
            status = r.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
