#!/usr/bin/env python3
"""Distance-estimate measurements (profiles/distance/README.md).

    python scripts/distance_rate.py launches   launch_view_distance, both designs (kernel "default" = two passes, "asm" = one
                                               pass), against launch_view_smooth on cfg2's and cfg5's views (4096^2), with the
                                               cycle test on and off: ms per launch, ratio to smooth, reference pixel-steps / s
    python scripts/distance_rate.py render     cfg5's view as a distance image at s = 1 and s = 2 beside the smooth render

Device buffers, one stream, HIP events around >= 50 ms of back-to-back launches after a warm-up, legs alternating within one
process.  Prints one JSON line per leg."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, Palette, View   # noqa: E402

VIEWS = {"cfg2": (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 1000), "cfg5": (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 5000)}


def timed(torch, fn, min_ms=50.0):
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


def launches():
    import torch
    px = 4096 * 4096
    dv = torch.empty(px, dtype=torch.float64, device="cuda:0")
    dc = torch.empty(px, dtype=torch.int32, device="cuda:0")
    for cycle in (1, 0):
        with MandelbrotDevice(0) as dev:
            dev.set_option("cycle_detect", cycle)
            for name, (view, mrd) in VIEWS.items():
                _, counts, st = dev.compute_view_smooth(view, mrd)
                esc_steps = int(counts[counts > 0].astype(np.int64).sum())
                legs = {"smooth": lambda: dev.launch_view_smooth(view, mrd, d_smooth=dv.data_ptr(), d_counts=dc.data_ptr()),
                        "counts": lambda: dev.launch_view(view, mrd, d_counts=dc.data_ptr()),
                        "distance_two_pass": lambda: dev.launch_view_distance(view, mrd, d_distance=dv.data_ptr(), d_counts=dc.data_ptr()),
                        "distance_one_pass": lambda: dev.launch_view_distance(view, mrd, d_distance=dv.data_ptr(), d_counts=dc.data_ptr(),
                                                                              kernel="asm"),
                        "smooth_asm": lambda: dev.launch_view_smooth(view, mrd, d_smooth=dv.data_ptr(), d_counts=dc.data_ptr(), kernel="asm")}
                ms = {}
                for _round in range(2):
                    for leg, fn in legs.items():
                        ms.setdefault(leg, []).append(timed(torch, fn))
                for leg, v in ms.items():
                    t = min(v)
                    print(json.dumps({"view": name, "cycle_detect": cycle, "leg": leg, "ms": round(t, 4), "ms_runs": [round(x, 4) for x in v],
                                      "ratio_to_smooth": round(t / min(ms["smooth"]), 3),
                                      "ref_pixel_steps_per_s": round(st.pixel_iterations / t * 1e3, 1),
                                      "escaped_pixel_steps": esc_steps}), flush=True)


def render():
    import torch
    view, mrd = VIEWS["cfg5"]
    d = torch.empty(4096 * 4096, dtype=torch.int32, device="cuda:0")
    with MandelbrotDevice(0) as dev:
        pals = {"smooth": Palette.cosine(1024), "distance": Palette.distance(view, 8.0)}
        for s in (1, 2):
            for source, pal in pals.items():
                t = timed(torch, lambda: dev.launch_render_view(view, mrd, palette=pal, d_rgba=d.data_ptr(), source=source, supersample=s))
                print(json.dumps({"render": source, "supersample": s, "ms": round(t, 3)}), flush=True)


if __name__ == "__main__":
    {"launches": launches, "render": render}[sys.argv[1] if len(sys.argv) > 1 else "launches"]()
