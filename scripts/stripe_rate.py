#!/usr/bin/env python3
"""Stripe-average measurements (profiles/stripe/README.md).

    python scripts/stripe_rate.py launches   launch_view_stripes at density 1, 5 and 16 beside launch_view, launch_view_smooth
                                             and launch_view_distance of the same build, on cfg5's view (4096^2, mrd 5000):
                                             ms per launch, ratios to the distance and the smooth launch
    python scripts/stripe_rate.py render     launch_render_view_stripes beside the relief and the smooth render, the same
                                             rectangle at 1024^2, supersample 2

Device buffers, one stream, HIP events around >= 200 ms of back-to-back launches after a warm-up (the clock is ramped by then),
the legs alternating within one process, each leg run three times: the lowest run is the figure, the three give the spread.
Before timing, the script checks at the size that is timed that the counts beside the stripe averages are the distance
launch's and that a value is 0 exactly where the count is.  Prints one JSON line per leg."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, Palette, View   # noqa: E402

CFG5 = (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 5000)
RENDER = (View(-2.0, -1.5, 3.0, 3.0, 1024, 1024), 5000)
ROUNDS = 3


def timed(torch, fn, min_ms=200.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    total, n = 0.0, 0
    while total < min_ms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
        n += 4
    return total / n


def run_legs(torch, legs):
    ms = {}
    for _round in range(ROUNDS):
        for leg, fn in legs.items():
            ms.setdefault(leg, []).append(timed(torch, fn))
    return ms


def launches():
    import torch
    view, mrd = CFG5
    px = view.width * view.height
    dv = torch.empty(px, dtype=torch.float64, device="cuda:0")
    dc = torch.empty(px, dtype=torch.int32, device="cuda:0")
    ds = torch.empty(4 * px, dtype=torch.float64, device="cuda:0")
    with MandelbrotDevice(0) as dev:
        _, counts, st = dev.compute_view_distance(view, mrd)
        c1, v1, _ = dev.compute_view_stripes(view, mrd, density=5)
        assert np.array_equal(c1, counts) and not np.isnan(v1).any() and np.array_equal(v1 == 0.0, counts == 0)
        del c1, v1
        p = {"d_counts": dc.data_ptr()}
        legs = {"counts": lambda: dev.launch_view(view, mrd, **p),
                "smooth": lambda: dev.launch_view_smooth(view, mrd, d_smooth=dv.data_ptr(), **p),
                "distance": lambda: dev.launch_view_distance(view, mrd, d_distance=dv.data_ptr(), **p)}
        for density in (1, 5, 16):
            legs[f"stripes_s{density}"] = lambda density=density: dev.launch_view_stripes(view, mrd, d_stripe=dv.data_ptr(), density=density, **p)
        legs["stripes_s5_with_state"] = lambda: dev.launch_view_stripes(view, mrd, d_stripe=dv.data_ptr(), d_state=ds.data_ptr(), density=5, **p)
        ms = run_legs(torch, legs)
        for leg, v in ms.items():
            t = min(v)
            print(json.dumps({"leg": leg, "ms": round(t, 4), "ms_runs": [round(x, 4) for x in v], "spread": round(max(v) / t - 1.0, 4),
                              "ratio_to_distance": round(t / min(ms["distance"]), 4), "ratio_to_smooth": round(t / min(ms["smooth"]), 4),
                              "second_pass_ms": round(t - min(ms["counts"]), 4),
                              "ref_pixel_steps": int(st.pixel_iterations), "never_pixels": int(st.never_pixels),
                              "escaped_pixel_steps": int(counts[counts > 0].astype(np.int64).sum())}), flush=True)


def render():
    import torch
    view, mrd = RENDER
    d = torch.empty(view.width * view.height, dtype=torch.int32, device="cuda:0")
    pal = Palette.cosine(1024)
    with MandelbrotDevice(0) as dev:
        kw = dict(palette=pal, d_rgba=d.data_ptr(), supersample=2)
        legs = {"smooth": lambda: dev.launch_render_view(view, mrd, source="smooth", **kw),
                "relief": lambda: dev.launch_render_view_relief(view, mrd, **kw)}
        for density in (1, 5, 16):
            legs[f"stripes_s{density}"] = lambda density=density: dev.launch_render_view_stripes(view, mrd, density=density, **kw)
        ms = run_legs(torch, legs)
        for leg, v in ms.items():
            t = min(v)
            print(json.dumps({"render": leg, "supersample": 2, "ms": round(t, 4), "ms_runs": [round(x, 4) for x in v],
                              "spread": round(max(v) / t - 1.0, 4), "ratio_to_smooth": round(t / min(ms["smooth"]), 3),
                              "ratio_to_relief": round(t / min(ms["relief"]), 3)}), flush=True)


if __name__ == "__main__":
    {"launches": launches, "render": render}[sys.argv[1] if len(sys.argv) > 1 else "launches"]()
