#!/usr/bin/env python3
"""rd_curve.py -- the MP half of Compression.cpp -g (:303-350): compression curves of image files or seeded synthetic frames.

    python tools/rd_curve.py [--K 32] [--fast] [--levels 8,7,6,5,4,3,2,1] [--csv out.csv] [--time] [--repeats 5]
                             [--json out.json] (FILE ... | --synthetic WxH[:seed] ...)

Writes the reference's CSV ("File, Mode, Quality, Size, BPP, PSNR", numbers as std::format("{}") prints them) from one
mpc_rate_distortion_device call per image.  --time: per image, mpc_rate_distortion_device against the composed loop
encode_image_device + decode_image + mpc_psnr over the same levels, the two alternated in one process, median and spread of
--repeats runs each; and the summed pursuit kernel time of the sweep (mpc_kernel_timing_read).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(spec):
    if spec.startswith("synthetic:"):
        from bench import synth_frame
        size, _, seed = spec[len("synthetic:"):].partition(":")
        W, H = (int(v) for v in size.split("x"))
        return synth_frame(W, H, int(seed or 12345))
    if spec.endswith(".mn"):
        import imageexperiments_amd as ia
        with open(spec, "rb") as f:
            return np.ascontiguousarray(ia.decode_image(f.read(), load.ctx))
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(spec).convert("RGB")))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="*")
    ap.add_argument("--synthetic", action="append", default=[], metavar="WxH[:seed]")
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--fast", action="store_true", help="the `...Fast` (float) flavour, what Compression.cpp itself runs")
    ap.add_argument("--levels", default="8,7,6,5,4,3,2,1", help="bpp allocations and/or 'max'")
    ap.add_argument("--csv", default=None, help="CSV output (default: stdout)")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None, help="timing results as JSON")
    a = ap.parse_args()
    import torch
    import imageexperiments_amd as ia
    ctx = ia.create_compression_context(a.K, 8, 3.5, device=0).set_fast(a.fast)
    load.ctx = ctx
    levels = [v if v == "max" else float(v) for v in a.levels.split(",")]
    names = list(a.files) + ["synthetic:" + s for s in a.synthetic]
    if not names:
        ap.error("no input")
    rows = ["File, Mode, Quality, Size, BPP, PSNR"]
    report = []
    fmt = ia.format_double
    for name in names:
        rgb = load(name)
        H, W = rgb.shape[:2]
        d_rgb = torch.from_numpy(rgb).cuda()
        torch.cuda.synchronize()
        points = ctx.rate_distortion_device(d_rgb.data_ptr(), W, H, levels)
        for p in points:
            q = "max" if p.quality == "max" else fmt(p.quality)
            rows.append(f"{name}, MP, {q}, {p.size}, {fmt(p.bpp)}, {fmt(p.psnr)}")
        if not a.time:
            continue
        _, quants = ia.parse_qualities(levels, a.K)

        def composed():
            for q in quants:
                blob = ctx.encode_image_device(d_rgb.data_ptr(), W, H, quant=q)
                ia.calculate_psnr(rgb, ia.decode_image(blob, ctx))

        def sweep():
            ctx.rate_distortion_device(d_rgb.data_ptr(), W, H, levels)

        sweep(), composed()                                        # warm: workspaces, staging, job buffers
        t_sweep, t_composed = [], []
        for _ in range(a.repeats):
            for fn, acc in ((sweep, t_sweep), (composed, t_composed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                acc.append(1e3 * (time.perf_counter() - t0))
        ctx.kernel_timing(True)
        pursuit = []
        for _ in range(a.repeats):
            sweep()
            pursuit.append(ctx.read_kernel_timing()[0])
        ctx.kernel_timing(False)
        r = {"file": name, "width": W, "height": H, "K": a.K, "fast": a.fast, "levels": [str(v) for v in levels],
             "rate_distortion_device_ms": spread(t_sweep), "composed_loop_ms": spread(t_composed), "pursuit_kernel_ms": spread(pursuit)}
        r["speedup_median"] = r["composed_loop_ms"]["median"] / r["rate_distortion_device_ms"]["median"]
        r["sweep_over_pursuit"] = r["rate_distortion_device_ms"]["median"] / r["pursuit_kernel_ms"]["median"]
        report.append(r)
        print(json.dumps(r), file=sys.stderr)
    text = "\n".join(rows) + "\n"
    if a.csv:
        with open(a.csv, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
