#!/usr/bin/env python3
"""patch_stream_timing.py -- the delta stream against whole containers, sender and receiver, on a frame sequence in which a fraction of
the tiles changes from frame to frame.
    python tools/patch_stream_timing.py [--out profiles/patch_stream.txt] [--runs 12] [--limit 300]
    python tools/patch_stream_timing.py --leg random:0.01         (one leg, in this process)
Workload and sequences: tools/delta_encode_timing.py's (4928x3264, K = 32, quality 3.5, device pixels; random and rectangle changes),
fractions 0, 1 %, 10 %, 50 %.  Two delta sessions are fed the same frames, one through mpc_delta_encode and one through
mpc_delta_encode_patch; per frame, alternating in one process, profiler off, the host clock around calls that return complete:
    sender    mpc_delta_encode | mpc_delta_encode_patch, and the bytes of both
    receiver  mpc_patch_apply of the patch | mpc_decode_image_device of the whole container | mpc_decode_images_indexed_device of the
              whole container with the index the encoder makes (the fastest whole-frame route)
Outside the clock the patch-applied frame is compared with the whole decode, byte for byte.  Then the unpack kernel alone, HIP events
around mpc_unpack_tiles_device on buffers of its own with the last frame's list.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from delta_encode_timing import H, K, QUALITY, W, synth_frame  # noqa: E402

FRACTIONS = (0.0, 0.01, 0.1, 0.5)
VARIANTS = ("random", "rectangle")


def leg(variant, fraction, runs):
    import numpy as np
    import torch
    import imageexperiments_amd as ia
    tx, ty = W // 8, H // 8
    tiles = tx * ty
    ctx = ia.create_compression_context(K, 8, QUALITY, device=0)
    d_a, d_b = (torch.from_numpy(synth_frame(np, W, H, seed)).cuda() for seed in (12345, 12346))
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
            first = (i % (tx // columns)) * columns
            side = np.zeros((ty, tx), bool)
            side[:, first:first + columns] = True

    def frame():
        mask = torch.from_numpy(side).cuda().repeat_interleave(8, 0).repeat_interleave(8, 1).unsqueeze(2)
        out = torch.where(mask, d_b, d_a).contiguous()
        torch.cuda.synchronize()
        return out

    whole_enc, patch_enc, dec = ctx.delta_encoder(W, H), ctx.delta_encoder(W, H), ctx.patch_decoder(W, H)
    out_whole = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    out_indexed = torch.empty(3 * W * H, dtype=torch.uint8, device="cuda")
    names = ("encode", "encode_patch", "apply", "decode", "decode_indexed")
    ms = {k: [] for k in names}
    size = {"whole": [], "patch": []}
    changed, routes = [], set()
    warm = 3
    for i in range(warm + runs):
        advance(i)
        cur = frame()
        got = {}

        def clocked(which, call):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got[which] = call()
            took = (time.perf_counter() - t) * 1e3
            if i >= warm:
                ms[which].append(took)

        send = (("encode", lambda: whole_enc.encode_device(cur.data_ptr())), ("encode_patch", lambda: patch_enc.encode_patch_device(cur.data_ptr())))
        for which, call in send if i % 2 == 0 else send[::-1]:
            clocked(which, call)
        blob, patch = got["encode"], got["encode_patch"]
        index = ia.container_index(blob, 0, expanded=True)          # byte for byte what mpc_delta_encode returns with an interval
        receive = (("apply", lambda: dec.apply(patch)), ("decode", lambda: ctx.decode_image_device(blob, out_whole)),
                   ("decode_indexed", lambda: ctx.decode_images_indexed_device([blob], [index], [out_indexed])))
        for which, call in [receive[(i + k) % 3] for k in range(3)]:
            clocked(which, call)
        assert whole_enc.info[:2] == patch_enc.info[:2] and (i == 0) == bool(patch_enc.info[2]), (variant, fraction, i, patch_enc.info)
        routes.update(got["decode_indexed"][1])                                          # 0 = parsed on the device
        applied = torch.from_numpy(dec.frame()).cuda().view(-1)
        assert bool((applied == out_whole).all()) and bool((out_indexed == out_whole).all()), (variant, fraction, i)
        if i >= warm:
            size["whole"].append(len(blob))
            size["patch"].append(len(patch))
            changed.append(patch_enc.info[1])
    # the unpack kernel alone: the last list, a packed frame of its size and a frame of their own
    listed = patch_enc.changed()
    us = [0.0]
    if 0 < listed.size < tiles:
        R, Cc, stride, nbytes = ia.delta_pack_geometry(listed.size)
        packed = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_list = torch.from_numpy(listed.copy()).cuda()
        dst = d_a.clone()
        stream = torch.cuda.current_stream().cuda_stream
        us = []
        for k in range(24):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            ctx.unpack_tiles_device(packed.data_ptr(), 0, d_list.data_ptr(), listed.size, 64, dst.data_ptr(), W, H, 0, stream, check=False)
            stop.record()
            stop.synchronize()
            if k >= 4:
                us.append(start.elapsed_time(stop) * 1e3)

    def show(k):
        return f"{statistics.median(ms[k]):6.2f} ms ({min(ms[k]):.2f} - {max(ms[k]):.2f})"

    print(f"{variant:9s} {100 * fraction:5.1f} %  changed {statistics.median(changed):8.0f} of {tiles}  "
          f"encode {show('encode')}  encode_patch {show('encode_patch')}  bytes {statistics.median(size['whole']):9.0f} | {statistics.median(size['patch']):9.0f}  "
          f"apply {show('apply')}  decode {show('decode')}  decode indexed {show('decode_indexed')} route {sorted(routes)}  "
          f"unpack {statistics.median(us):6.1f} us ({min(us):.1f} - {max(us):.1f})", flush=True)
    for s in (whole_enc, patch_enc, dec):
        s.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, help="variant:fraction, e.g. random:0.01")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=300, help="seconds a leg's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        variant, fraction = args.leg.split(":")
        leg(variant, float(fraction), args.runs)
        return 0
    lines = [f"# {W}x{H} K={K} quality {QUALITY}, device pixels; per frame, median (range) of {args.runs} frames, alternating in one process; "
             "encode = mpc_delta_encode, encode_patch = mpc_delta_encode_patch (two sessions, the same frames); bytes: container | patch; "
             "apply = mpc_patch_apply, decode = mpc_decode_image_device, decode indexed = mpc_decode_images_indexed_device, of the whole container; "
             "unpack = mp_tile_unpack_kernel, HIP events"]
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
