#!/usr/bin/env python3
"""Relief-shading measurements (profiles/relief/README.md), all on cfg5's view (4096^2, mrd 5000).

    python scripts/relief_rate.py launches   launch_view_normals against launch_view_distance of the same view, both designs
                                             (kernel "default" = two passes, "asm" = one pass), and the normals with the
                                             distance estimates beside them: ms per launch, ratio to the distance launch
    python scripts/relief_rate.py render     render_view_relief against render_view(source="smooth") and
                                             render_view(source="distance") at s = 1 and s = 2

Device buffers, one stream, HIP events around >= 200 ms of back-to-back launches after a warm-up, the legs alternating within
one process, each leg run three times: the lowest run is the figure, the three give the spread.  Before timing, the script
checks at the size that is timed that the two designs store the same normals and that the distance estimates beside the
normals are launch_view_distance's bits.  Prints one JSON line per leg."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, Palette, View   # noqa: E402

CFG5 = (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 5000)
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
    dn = torch.empty(2 * px, dtype=torch.float64, device="cuda:0")
    dv = torch.empty(px, dtype=torch.float64, device="cuda:0")
    dc = torch.empty(px, dtype=torch.int32, device="cuda:0")
    with MandelbrotDevice(0) as dev:
        de_ref, counts, st = dev.compute_view_distance(view, mrd)
        c1, n1, d1, _ = dev.compute_view_normals(view, mrd, want_distance=True)
        c2, n2, _ = dev.compute_view_normals(view, mrd, kernel="asm")
        assert np.array_equal(c1, counts) and np.array_equal(c2, counts)
        assert np.array_equal(n1.view(np.uint64), n2.view(np.uint64)) and np.array_equal(d1.view(np.uint64), de_ref.view(np.uint64))
        assert not np.isnan(n1).any() and np.array_equal((n1 != 0.0).any(axis=2), counts > 0)
        del de_ref, c1, n1, d1, c2, n2
        p = {"d_counts": dc.data_ptr()}
        legs = {"distance_two_pass": lambda: dev.launch_view_distance(view, mrd, d_distance=dv.data_ptr(), **p),
                "normals_two_pass": lambda: dev.launch_view_normals(view, mrd, d_normals=dn.data_ptr(), **p),
                "normals_and_distance_two_pass": lambda: dev.launch_view_normals(view, mrd, d_normals=dn.data_ptr(),
                                                                                 d_distance=dv.data_ptr(), **p),
                "counts": lambda: dev.launch_view(view, mrd, **p),
                "distance_one_pass": lambda: dev.launch_view_distance(view, mrd, d_distance=dv.data_ptr(), kernel="asm", **p),
                "normals_one_pass": lambda: dev.launch_view_normals(view, mrd, d_normals=dn.data_ptr(), kernel="asm", **p)}
        ms = run_legs(torch, legs)
        for leg, v in ms.items():
            t = min(v)
            base = min(ms["distance_one_pass" if leg.endswith("one_pass") else "distance_two_pass"])
            print(json.dumps({"leg": leg, "ms": round(t, 4), "ms_runs": [round(x, 4) for x in v],
                              "spread": round(max(v) / t - 1.0, 4), "ratio_to_distance": round(t / base, 4),
                              "ref_pixel_steps": int(st.pixel_iterations), "never_pixels": int(st.never_pixels),
                              "escaped_pixel_steps": int(counts[counts > 0].astype(np.int64).sum())}), flush=True)


def render():
    import torch
    view, mrd = CFG5
    d = torch.empty(view.width * view.height, dtype=torch.int32, device="cuda:0")
    smooth = Palette.cosine(1024)
    distance = Palette.distance(view, 8.0)
    with MandelbrotDevice(0) as dev:
        for s in (1, 2):
            legs = {"smooth": lambda: dev.launch_render_view(view, mrd, palette=smooth, d_rgba=d.data_ptr(), source="smooth", supersample=s),
                    "distance": lambda: dev.launch_render_view(view, mrd, palette=distance, d_rgba=d.data_ptr(), source="distance",
                                                               supersample=s),
                    "relief": lambda: dev.launch_render_view_relief(view, mrd, palette=smooth, d_rgba=d.data_ptr(), supersample=s)}
            ms = run_legs(torch, legs)
            for leg, v in ms.items():
                t = min(v)
                print(json.dumps({"render": leg, "supersample": s, "ms": round(t, 3), "ms_runs": [round(x, 3) for x in v],
                                  "spread": round(max(v) / t - 1.0, 4), "ratio_to_smooth": round(t / min(ms["smooth"]), 3),
                                  "ratio_to_distance": round(t / min(ms["distance"]), 3)}), flush=True)


if __name__ == "__main__":
    {"launches": launches, "render": render}[sys.argv[1] if len(sys.argv) > 1 else "launches"]()
