#!/usr/bin/env python3
"""rate_stream_timing.py -- the delta stream to a byte budget against the unbudgeted delta stream, on the sequences of
tools/patch_stream_timing.py (1 %, 10 %, 50 % of the tiles changing per frame, random and a moving rectangle) and on a scene cut
followed by a static tail.
    python tools/rate_stream_timing.py [--out profiles/rate_stream.txt] [--runs 12] [--limit 400]
    python tools/rate_stream_timing.py --leg random:0.1          (one leg, in this process)
4928x3264, K = 32, quality 3.5, device pixels, profiler off, everything warmed up.  A leg first runs its sequence through
mpc_delta_encode_patch alone to find the median patch size; the budgets are 1/4, 1/2 and 1x of it (the scene cut: of the cut frame's
own patch, the only one of its sequence that is not empty).  Then, per budget, twin sessions get the same frames, alternating in one
process with the host clock around calls that return complete: mpc_delta_encode_patch (the baseline: code this feature does not
touch) and mpc_delta_encode_patch_budget, each with a receiver of its own.  Per leg and budget: ms per call of both, probes, patch
bytes, the budget receiver's PSNR against the source frame and against the unbudgeted receiver's frame, and how many calls of a static
tail (the last frame again, 32 at most) it takes to reach owed == 0.  Medians and ranges of --runs frames.
Without --leg every leg runs in a fresh child process under its own `timeout`; the first failure stops the script, and the collected
lines go to --out."""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from delta_encode_timing import H, K, QUALITY, W, synth_frame  # noqa: E402

LEGS = [f"{v}:{f}" for v in ("random", "rectangle") for f in (0.01, 0.1, 0.5)] + ["cut:1.0"]
SHARES = (0.25, 0.5, 1.0)
TAIL = 32


def leg(variant, fraction, runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    tx, ty = W // 8, H // 8
    tiles = tx * ty
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    d_a, d_b = (torch.from_numpy(synth_frame(np, W, H, seed)).cuda() for seed in (12345, 12346))
    columns = max(int(round(fraction / 2 * tx)), 1)
    warm = 3

    def frames():
        """the sequence, the same on every pass: warm + runs frames"""
        rng = np.random.default_rng(7)
        side = np.zeros((ty, tx), bool)                              # True: the tile shows B
        for i in range(warm + runs):
            if variant == "random":
                swap = np.zeros(tiles, bool)
                swap[rng.choice(tiles, int(round(fraction * tiles)), replace=False)] = True
                side = side ^ swap.reshape(ty, tx)
            elif variant == "rectangle":
                first = (i % (tx // columns)) * columns
                side = np.zeros((ty, tx), bool)
                side[:, first:first + columns] = True
            else:                                                    # the scene cut: A while warming up, then B for good
                side = np.full((ty, tx), i >= warm)
            mask = torch.from_numpy(side).cuda().repeat_interleave(8, 0).repeat_interleave(8, 1).unsqueeze(2)
            out = torch.where(mask, d_b, d_a).contiguous()
            torch.cuda.synchronize()
            yield i, out

    def psnr(a, b):
        mse = float(((a.float() - b.float()) ** 2).mean())
        return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)

    # the unbudgeted stream alone: the sizes the budgets are shares of
    enc = ctx.delta_encoder(W, H)
    sizes = [len(enc.encode_patch_device(cur.data_ptr())) for i, cur in frames()][warm:]
    enc.close()
    basis = sizes[0] if variant == "cut" else statistics.median(sizes)
    print(f"{variant:9s} {100 * fraction:5.1f} %  unbudgeted patch bytes: median {statistics.median(sizes):.0f} ({min(sizes)} - {max(sizes)}); "
          f"budgets are shares of {basis:.0f}", flush=True)

    def show(v, unit="ms"):
        return f"{statistics.median(v):8.2f} {unit} ({min(v):.2f} - {max(v):.2f})"

    for share in SHARES:
        budget = int(math.ceil(share * basis))
        plain, rated = ctx.delta_encoder(W, H), ctx.delta_encoder(W, H)
        rx_plain, rx_rated = ctx.patch_decoder(W, H), ctx.patch_decoder(W, H)
        ms = {"plain": [], "rated": []}
        probes, nbytes, owed, sent, to_source, to_plain, refused = [], [], [], [], [], [], None
        cur = None
        for i, cur in frames():
            got = {}

            def clocked(which, call):
                torch.cuda.synchronize()
                t = time.perf_counter()
                got[which] = call()
                if i >= warm:
                    ms[which].append((time.perf_counter() - t) * 1e3)

            # the warm-up frames are sent whole: the budgets are about the steady stream (and the cut), not about the first key frame
            room = 1 << 40 if i < warm else budget
            calls = (("plain", lambda: plain.encode_patch_device(cur.data_ptr())), ("rated", lambda: rated.encode_patch_budget_device(cur.data_ptr(), room)))
            try:
                for which, call in calls if i % 2 == 0 else calls[::-1]:
                    clocked(which, call)
            except ia.MpcError as e:
                refused = str(e)
                break
            patch, info = got["rated"]
            assert len(patch) <= room
            rx_plain.apply(got["plain"])
            rx_rated.apply(patch)
            if i >= warm:
                f_plain, f_rated = (torch.from_numpy(r.frame()).cuda() for r in (rx_plain, rx_rated))
                probes.append(info.probes)
                nbytes.append(len(patch))
                owed.append(info.owed)
                sent.append(info.sent_tiles)
                to_source.append(psnr(f_rated, cur))
                to_plain.append(psnr(f_rated, f_plain))
        if refused:
            print(f"    budget {share:4.2f}x = {budget:9d} B  refused: {refused}", flush=True)
        else:
            # the static tail: the last frame again until nothing is owed
            tail, tail_ms = None, []
            left = owed[-1]
            for k in range(TAIL):
                if left == 0:
                    tail = k
                    break
                torch.cuda.synchronize()
                t = time.perf_counter()
                patch, info = rated.encode_patch_budget_device(cur.data_ptr(), budget)
                tail_ms.append((time.perf_counter() - t) * 1e3)
                rx_rated.apply(patch)
                left = info.owed
            else:
                tail = TAIL if left == 0 else None
            reached = f"{tail} calls" if tail is not None else f"not within {TAIL} calls ({left} of {tiles} tiles still owed)"
            end = psnr(torch.from_numpy(rx_rated.frame()).cuda(), cur)
            print(f"    budget {share:4.2f}x = {budget:9d} B  encode_patch {show(ms['plain'])}  encode_patch_budget {show(ms['rated'])}  "
                  f"probes {statistics.median(probes):.0f} ({min(probes)} - {max(probes)})  bytes {statistics.median(nbytes):9.0f} ({min(nbytes)} - {max(nbytes)})  "
                  f"sent tiles {statistics.median(sent):8.0f}  owed {statistics.median(owed):8.0f} (last {owed[-1]})  "
                  f"PSNR to source {show(to_source, 'dB')}  to the unbudgeted receiver {show(to_plain, 'dB')}  "
                  f"static tail to owed == 0: {reached}{'' if not tail_ms else f', {statistics.median(tail_ms):.2f} ms a call'}, PSNR to source then {end:.2f} dB",
                  flush=True)
        for s in (plain, rated, rx_plain, rx_rated):
            s.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, help="variant:fraction, e.g. random:0.01; cut:1.0 is the scene cut")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=400, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        variant, fraction = args.leg.split(":")
        leg(variant, float(fraction), args.runs)
        return 0
    lines = [f"# {W}x{H} K={K} quality {QUALITY}, device pixels; per frame, median (range) of {args.runs} frames, twin sessions alternating in one "
             "process; encode_patch = mpc_delta_encode_patch (the baseline), encode_patch_budget = mpc_delta_encode_patch_budget; budgets are shares of "
             "the sequence's median unbudgeted patch (the scene cut: of the cut frame's patch); the warm-up frames are sent whole"]
    print(lines[0], flush=True)
    status = 0
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--runs", str(args.runs)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
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
