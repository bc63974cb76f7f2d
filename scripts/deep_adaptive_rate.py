#!/usr/bin/env python3
"""Adaptive supersampling of deep views: measurements (profiles/deep_adaptive/README.md).

    python scripts/deep_adaptive_rate.py [--size 4096] [--rounds 3] [--out FILE]

The seahorse-valley view at span 1e-20, mrd 30000 (profiles/deep/), source smooth, Palette.cosine(period=--period):
render_deep_view at s = 1, 2, 4, 8 and render_deep_view_adaptive at s = 2, 4, 8, with bla off and on.  The threshold is the one
of THRESHOLDS whose refined share (the mask's mean; read at s = 1, where no fine sample is computed) lies nearest 15 %.

Legs alternate within one process after a clock ramp; a leg lasts >= 50 ms and >= 3 calls after a warm-up call -- a call of a
second or more IS longer than any ramp and is timed as it stands, once per round.  Per leg: wall per call and the call's
kernel_ms (device events around its kernels), medians over the rounds, and the call's pixel_iterations (the stored counts of
the samples it computed: the same every call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--period", type=float, default=1500.0, help="units of nu per turn of the palette")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, Palette   # noqa: E402

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
SPAN, MRD = 1e-20, 30000
FACTORS = (2, 4, 8)
THRESHOLDS = (4, 8, 16, 32, 64, 96, 128, 160, 200)
LONG_CALL = 1.0   # seconds


def leg(fn, min_seconds=0.05, min_calls=3):
    """(wall seconds per call, median kernel_ms of the calls)"""
    t0 = time.perf_counter()
    first = fn()
    dt = time.perf_counter() - t0
    if dt >= LONG_CALL:
        return dt, float(first)
    n, kernel, t0 = 0, [], time.perf_counter()
    while True:
        kernel.append(fn())
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= min_calls:
            return dt / n, float(np.median(kernel))


def main():
    n = args.size
    orbit = DeepOrbit(*SEAHORSE, MRD, min_span=SPAN)
    view = DeepView(SPAN, n, n)
    pal = Palette.cosine(period=args.period)
    result = {"size": n, "span": SPAN, "mrd": MRD, "period": args.period, "orbit_length": orbit.length, "legs": {},
              "refined_share": {}, "pixel_iterations": {}}
    iters = result["pixel_iterations"]

    def timed(key, st):
        iters[key] = int(st.pixel_iterations)
        return st.kernel_ms

    with MandelbrotDevice(0) as dev:
        result["device"] = dev.info()["name"]
        rgba = dev.pinned_empty((n, n, 4), np.uint8)
        for bla in (False, True):
            for thr in THRESHOLDS:
                _, mask, _ = dev.render_deep_view_adaptive(orbit, view, MRD, palette=pal, supersample=1, threshold=thr, want_mask=True,
                                                           bla=bla)
                result["refined_share"][f"{'bla' if bla else 'plain'}_t{thr}"] = float(mask.mean())
        thr = min(THRESHOLDS, key=lambda t: abs(result["refined_share"][f"plain_t{t}"] - 0.15))
        result["threshold"] = thr
        print("refined share:", result["refined_share"], "-> threshold", thr, flush=True)
        legs = {}

        def add(key, call):
            legs[key] = lambda: timed(key, call()[1])

        for bla in (False, True):
            tag = "bla" if bla else "plain"
            for s in (1,) + FACTORS:
                add(f"{tag}_render_s{s}", lambda s=s, bla=bla: dev.render_deep_view(
                    orbit, view, MRD, palette=pal, supersample=s, out=rgba, bla=bla))
            for s, t in [(s, thr) for s in FACTORS] + [(2, 256)]:
                add(f"{tag}_adaptive_s{s}_t{t}", lambda s=s, t=t, bla=bla: dev.render_deep_view_adaptive(
                    orbit, view, MRD, palette=pal, supersample=s, threshold=t, out=rgba, bla=bla))
        for _ in range(3):   # clock ramp
            legs["plain_render_s1"]()
        rounds = {k: [] for k in legs}
        for r in range(args.rounds):
            for k, fn in legs.items():
                rounds[k].append(leg(fn))
            print("round", r + 1, "of", args.rounds, "done", flush=True)
        for k, v in rounds.items():
            wall = sorted(1e3 * w for w, _ in v)
            kern = sorted(km for _, km in v)
            result["legs"][k] = {"wall_ms_median": float(np.median(wall)), "wall_ms_min": wall[0], "wall_ms_max": wall[-1],
                                 "kernel_ms_median": float(np.median(kern)), "kernel_ms_min": kern[0], "kernel_ms_max": kern[-1]}
            print(f"{k:28s} wall {np.median(wall):10.3f} ms ({wall[0]:.3f} .. {wall[-1]:.3f})   kernels {np.median(kern):10.3f} ms "
                  f"({kern[0]:.3f} .. {kern[-1]:.3f})", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
