#!/usr/bin/env python3
"""patch_index_timing.py -- version-1 against version-2 patches of the same frames: what the seek index in a patch costs the sender and
saves the receiver.
    python tools/patch_index_timing.py [--out profiles/patch_index.txt] [--runs 12] [--limit 420]
    python tools/patch_index_timing.py --leg 4928x3264x32         (one frame size with all its cases, in this process)
Frame sizes 4928x3264 at K = 32 and 1920x1080 at K = 8, quality 3.5, device pixels; frames as tools/delta_encode_timing.py makes them
(A with B's pixels in a set of tiles, a fresh random set of `share` of the tiles swapping sides from frame to frame).  Cases: changed
shares 0.1, 1, 3, 10 and 50 %, and "key" (every call a key frame, half of the tiles swapping in between).  Two sender sessions are fed
the same frames, one through mpc_delta_encode_patch and one through mpc_delta_encode_patch_indexed (the default interval,
index_min_bytes 0), and two receiver sessions apply the version-1 and the version-2 patch; per frame, alternating in one process,
profiler off, the host clock around calls that return complete.  Outside the clock: the version-2 patch is mpc_patch_add_index of the
version-1 patch, its route is 0, and the two kept frames are equal byte for byte.
Without --leg every frame size runs in a fresh child process under its own `timeout`; the first failure stops the script, and the
collected lines go to --out."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from delta_encode_timing import QUALITY, synth_frame  # noqa: E402

SIZES = ("4928x3264x32", "1920x1080x8")
CASES = (0.001, 0.01, 0.03, 0.1, 0.5, "key")
WARM = 3


def leg(size, runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    W, H, K = (int(v) for v in size.split("x"))
    tx, ty = -(-W // 8), -(-H // 8)
    tiles = tx * ty
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    d_a, d_b = (torch.from_numpy(synth_frame(np, W, H, seed)).cuda() for seed in (12345, 12346))
    for case in CASES:
        share = 0.5 if case == "key" else case
        rng = np.random.default_rng(7)
        side = np.zeros((ty, tx), bool)                              # True: the tile shows B
        plain, indexed = ctx.delta_encoder(W, H), ctx.delta_encoder(W, H)
        one, two = ctx.patch_decoder(W, H), ctx.patch_decoder(W, H)
        names = ("send 1", "send 2", "apply 1", "apply 2")
        ms = {k: [] for k in names}
        nbytes, index_bytes, container_bytes, changed, routes = [], [], [], [], set()
        for i in range(WARM + runs):
            swap = np.zeros(tiles, bool)
            swap[rng.choice(tiles, max(int(round(share * tiles)), 1), replace=False)] = True
            side = side ^ swap.reshape(ty, tx)
            mask = torch.from_numpy(side).cuda().repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W].unsqueeze(2)
            cur = torch.where(mask, d_b, d_a).contiguous()
            key = case == "key"
            got = {}

            def clocked(which, call):
                torch.cuda.synchronize()
                t = time.perf_counter()
                got[which] = call()
                took = (time.perf_counter() - t) * 1e3
                if i >= WARM:
                    ms[which].append(took)

            send = (("send 1", lambda: plain.encode_patch_device(cur.data_ptr(), key=key)),
                    ("send 2", lambda: indexed.encode_patch_device(cur.data_ptr(), key=key, index_interval=0, index_min_bytes=0)))
            for which, call in send if i % 2 == 0 else send[::-1]:
                clocked(which, call)
            p1, p2 = got["send 1"], got["send 2"]
            receive = (("apply 1", lambda: one.apply(p1)), ("apply 2", lambda: two.apply(p2)))
            for which, call in receive if i % 2 == 0 else receive[::-1]:
                clocked(which, call)
            assert p2 == ia.patch_add_index(p1, 0), (size, case, i)
            assert one.last_route() == 1
            routes.add(two.last_route())
            if i >= WARM:
                nbytes.append(len(p2))
                index_bytes.append(ia.patch_index(p2)[1])
                container_bytes.append(ia.patch_info(p2)["container_bytes"])
                changed.append(plain.info[1])
        assert (one.frame() == two.frame()).all(), (size, case)

        def show(k):
            return f"{statistics.median(ms[k]):6.2f} ms ({min(ms[k]):.2f} - {max(ms[k]):.2f})"

        label = "key    " if case == "key" else f"{100 * case:5.1f} %"
        print(f"{size:13s} {label}  changed {statistics.median(changed):8.0f} of {tiles}  apply v1 {show('apply 1')}  apply v2 {show('apply 2')} "
              f"route {sorted(routes)}  container {statistics.median(container_bytes):9.0f} bytes  patch v2 {statistics.median(nbytes):9.0f} bytes, index {100 * statistics.median(index_bytes) / statistics.median(nbytes):4.1f} %  "
              f"send v1 {show('send 1')}  send v2 {show('send 2')}", flush=True)
        for s in (plain, indexed, one, two):
            s.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, help="WxHxK, e.g. 4928x3264x32")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=420, help="seconds a frame size's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.runs)
        return 0
    lines = [f"# quality {QUALITY}, device pixels, random changes; per frame, median (range) of {args.runs} frames, version 1 and version 2 alternating "
             "in one process, profiler off; apply = mpc_patch_apply of the version-1 | version-2 patch of the same frame (two receivers); route = "
             "mpc_patch_last_route of the version-2 applies; send = mpc_delta_encode_patch | mpc_delta_encode_patch_indexed (default interval, "
             "index_min_bytes 0; two senders)"]
    print(lines[0], flush=True)
    status = 0
    for size in SIZES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", size, "--runs", str(args.runs)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines += r.stdout.splitlines()
        if r.returncode != 0:                                       # the first failure ends the script: nothing more is started
            sys.stderr.write(r.stderr[-4000:])
            lines.append(f"# {size} ended with status {r.returncode}; nothing was run after it")
            status = r.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
