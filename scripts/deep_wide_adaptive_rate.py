#!/usr/bin/env python3
"""Adaptive supersampling of extended-range deep views: measurements (profiles/deep_wide_adaptive/README.md).

    python scripts/deep_wide_adaptive_rate.py [--view i-1100|mis-1100] [--size 5632] [--rounds 3] [--out FILE]

The views of tests/test_deep_wide.py at range 1.0, exp2 -1100: c = i at mrd 3000 and the Misiurewicz point of the period-3
antenna at mrd 4000; source smooth, Palette.cosine(1000, period=--period).  render_deep_view at s = 1, 2, 4, 8 and
render_wide_view_adaptive at s = 2, 4, 8, with xbla off and on.  The threshold is the one of THRESHOLDS whose refined share (the
mask's mean; read at s = 1, where no fine sample is computed) lies nearest 15 %.

Legs alternate within one process after a clock ramp; a leg lasts >= 250 ms and >= 3 calls after a warm-up call (with xbla a
call at s = 1 is a few milliseconds: the leg repeats it) -- a call of a second or more IS longer than any ramp and is timed as
it stands, once per round.  Per leg: wall per call and the call's kernel_ms (device events around its kernels), medians over the
rounds, and the call's pixel_iterations (the stored counts of the samples it computed: the same every call).  Per s the result
also holds adaptive / (t(1) + share x t(s)) and the refine kernel's rate beside the full render's."""
import argparse
import json
import os
import sys
import time
from decimal import Decimal, getcontext

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--view", default="i-1100", choices=("i-1100", "mis-1100"))
ap.add_argument("--size", type=int, default=5632, help="W = H; W x 8 squared must stay below the 2^31 samples of a window")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--period", type=float, default=7.3, help="units of nu per turn of the palette")
ap.add_argument("--factors", default="2,4,8")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, Palette, WideDeepView   # noqa: E402

EXP2 = -1100
FACTORS = tuple(int(x) for x in args.factors.split(","))
THRESHOLDS = (1, 2, 4, 8, 16, 32, 64, 96, 128, 160, 200)
LONG_CALL = 1.0   # seconds


def misiurewicz() -> str:
    """The real root of c^3 + 2c^2 + 2c + 2 to 1300 digits, by Newton (tests/test_deep_wide.py's MIS)."""
    getcontext().prec = 1320
    c = Decimal("-1.5436890126920763615708559718")
    for _ in range(12):
        c = c - (((c + 2) * c + 2) * c + 2) / ((3 * c + 4) * c + 2)
    return str(c.quantize(Decimal(10) ** -1300))


def leg(fn, min_seconds=0.25, min_calls=3):
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
    centre, mrd = (("0", "1"), 3000) if args.view == "i-1100" else ((misiurewicz(), "0"), 4000)
    view = WideDeepView(1.0, EXP2, n, n)
    orbit = DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)
    pal = Palette.cosine(1000, period=args.period)
    result = {"view": args.view, "size": n, "exp2": EXP2, "mrd": mrd, "period": args.period, "orbit_length": orbit.length,
              "legs": {}, "refined_share": {}, "pixel_iterations": {}, "ratios": {}}
    iters = result["pixel_iterations"]

    def timed(key, st):
        iters[key] = int(st.pixel_iterations)
        return st.kernel_ms

    with MandelbrotDevice(0) as dev:
        result["device"] = dev.info()["name"]
        rgba = dev.pinned_empty((n, n, 4), np.uint8)
        for xbla in (False, True):
            for thr in THRESHOLDS:
                _, mask, _ = dev.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=1, threshold=thr, want_mask=True,
                                                           xbla=xbla)
                result["refined_share"][f"{'xbla' if xbla else 'plain'}_t{thr}"] = float(mask.mean())
        thr = min(THRESHOLDS, key=lambda t: abs(result["refined_share"][f"plain_t{t}"] - 0.15))
        result["threshold"] = thr
        print("refined share:", result["refined_share"], "-> threshold", thr, flush=True)
        legs = {}

        def add(key, call):
            legs[key] = lambda: timed(key, call()[1])

        for xbla in (False, True):
            tag = "xbla" if xbla else "plain"
            for s in (1,) + FACTORS:
                add(f"{tag}_render_s{s}", lambda s=s, xbla=xbla: dev.render_deep_view(
                    orbit, view, mrd, palette=pal, supersample=s, out=rgba, xbla=xbla))
            for s, t in [(s, thr) for s in FACTORS] + [(2, 256)]:
                add(f"{tag}_adaptive_s{s}_t{t}", lambda s=s, t=t, xbla=xbla: dev.render_wide_view_adaptive(
                    orbit, view, mrd, palette=pal, supersample=s, threshold=t, out=rgba, xbla=xbla))
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
        for tag in ("plain", "xbla"):
            share = result["refined_share"][f"{tag}_t{thr}"]
            t1 = result["legs"][f"{tag}_render_s1"]["wall_ms_median"]
            for s in FACTORS:
                ts = result["legs"][f"{tag}_render_s{s}"]["wall_ms_median"]
                ta = result["legs"][f"{tag}_adaptive_s{s}_t{thr}"]["wall_ms_median"]
                # the refine kernel's rate in stored counts per second beside the full render's
                refine = (iters[f"{tag}_adaptive_s{s}_t{thr}"] - iters[f"{tag}_render_s1"]) / max(ta - t1, 1e-9) / 1e9
                full = iters[f"{tag}_render_s{s}"] / ts / 1e9
                result["ratios"][f"{tag}_s{s}"] = {"adaptive_over_full": ta / ts, "model_ms": t1 + share * ts,
                                                   "adaptive_over_model": ta / (t1 + share * ts),
                                                   "refine_Tcounts_per_s": refine, "full_Tcounts_per_s": full}
                print(f"{tag} s = {s}: adaptive / full {ta / ts:.3f}   t(1) + share x t(s) = {t1 + share * ts:.1f} ms   "
                      f"adaptive / that {ta / (t1 + share * ts):.3f}   refine {refine:.3f} T counts/s, full {full:.3f}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
