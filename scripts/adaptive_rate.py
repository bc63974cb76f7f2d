#!/usr/bin/env python3
"""Adaptive supersampling measurements (profiles/adaptive/README.md).

    python scripts/adaptive_rate.py wall [--out FILE]            render_view at s = 1, 2, 4, 8 and render_view_adaptive at
                                                                 s = 2, 4, 8 x thresholds 0, 8, 32, 256 (cfg5's view, 4096^2)
    python scripts/adaptive_rate.py wall --root DIR --plain      the render_view legs alone from the package under DIR (a
                                                                 checkout of the parent commit, built): the yardstick

    python scripts/adaptive_rate.py kernels                      six adaptive renders at s = 4, threshold 32 -- run under
                                                                 `rocprofv3 --kernel-trace --stats --output-format csv` for
                                                                 the classify and refine kernels' own times

Legs alternate within one process and each lasts >= 50 ms and >= 3 calls after a warm-up call, a clock ramp first, five rounds,
medians -- as scripts/render_rate.py does it.  Per leg: wall per call and the call's kernel_ms (device events around its
kernels).  kernel = asm runs the refine kernel on the per-step loop (the default: 8-step groups with the cycle test)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["wall", "kernels"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--plain", action="store_true", help="render_view legs only")
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from distributedmandelbrot_amd import MandelbrotDevice, Palette, View   # noqa: E402

MRD = 5000
FACTORS = (2, 4, 8)
THRESHOLDS = (0, 8, 32, 256)


def leg(fn, min_seconds=0.05, min_calls=3):
    """(wall seconds per call, median kernel_ms of the calls)"""
    fn()
    n, kernel, t0 = 0, [], time.perf_counter()
    while True:
        kernel.append(fn())
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= min_calls:
            return dt / n, float(np.median(kernel))


def main():
    view = View(-2.0, -1.5, 3.0, 3.0, args.size, args.size)
    pal = Palette.cosine()
    result = {"root": os.path.abspath(args.root), "size": args.size, "mrd": MRD, "legs": {}, "refined_share": {}}
    with MandelbrotDevice(0) as dev:
        result["device"] = dev.info()["name"]
        rgba = dev.pinned_empty((args.size, args.size, 4), np.uint8)
        legs = {}
        for s in (1,) + FACTORS:
            legs[f"render_view_s{s}"] = lambda s=s: dev.render_view(view, MRD, palette=pal, supersample=s, out=rgba)[1].kernel_ms
        if not args.plain:
            for s in FACTORS:
                for thr in THRESHOLDS:
                    legs[f"adaptive_s{s}_t{thr}"] = lambda s=s, thr=thr: dev.render_view_adaptive(
                        view, MRD, palette=pal, supersample=s, threshold=thr, out=rgba)[1].kernel_ms
                    if thr in (8, 32):
                        legs[f"adaptive_s{s}_t{thr}_asm"] = lambda s=s, thr=thr: dev.render_view_adaptive(
                            view, MRD, palette=pal, supersample=s, threshold=thr, kernel="asm", out=rgba)[1].kernel_ms
            legs["render_view_s2_asm"] = lambda: dev.render_view(view, MRD, palette=pal, supersample=2, kernel="asm", out=rgba)[1].kernel_ms
            for thr in THRESHOLDS:
                _, mask, _ = dev.render_view_adaptive(view, MRD, palette=pal, supersample=2, threshold=thr, want_mask=True)
                result["refined_share"][str(thr)] = float(mask.mean())
        for _ in range(3):   # clock ramp
            legs["render_view_s1"]()
        rounds = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                rounds[k].append(leg(fn))
        for k, v in rounds.items():
            wall = sorted(1e3 * w for w, _ in v)
            kern = sorted(km for _, km in v)
            result["legs"][k] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": wall[0], "wall_ms_max": wall[-1],
                                 "kernel_ms_median": float(np.median(kern)), "kernel_ms_min": kern[0], "kernel_ms_max": kern[-1]}
            print(f"{k:28s} wall {np.median(wall):9.3f} ms ({wall[0]:.3f} .. {wall[-1]:.3f})   kernels {np.median(kern):9.3f} ms "
                  f"({kern[0]:.3f} .. {kern[-1]:.3f})", flush=True)
    print("refined share:", result["refined_share"])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


def kernels():
    view = View(-2.0, -1.5, 3.0, 3.0, args.size, args.size)
    pal = Palette.cosine()
    with MandelbrotDevice(0) as dev:
        rgba = dev.pinned_empty((args.size, args.size, 4), np.uint8)
        for _ in range(6):
            dev.render_view_adaptive(view, MRD, palette=pal, supersample=4, threshold=32, out=rgba)


if __name__ == "__main__":
    main() if args.mode == "wall" else kernels()
