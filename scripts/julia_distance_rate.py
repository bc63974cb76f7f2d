#!/usr/bin/env python3
"""Julia distance-estimate measurements (profiles/julia_distance/README.md).

    python scripts/julia_distance_rate.py     launch_julia_view_distance, both designs (kernel "default" = two passes, "asm" =
                                              one pass), against launch_julia_view with smooth output of the same view
                                              (4096^2, mrd 1000) for c = -0.75 (connected, with interior), c = i (a dendrite)
                                              and c = -0.8 + 0.156i (a dust): ms per launch, ratio to smooth

Device buffers, one stream, HIP events around >= 50 ms of back-to-back launches after a warm-up, legs alternating within one
process, each leg run twice.  Prints one JSON line per leg."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, View   # noqa: E402

VIEW, MRD = View(-1.6, -1.6, 3.2, 3.2, 4096, 4096), 1000
PARAMETERS = {"-0.75": (-0.75, 0.0), "i": (0.0, 1.0), "-0.8+0.156i": (-0.8, 0.156)}


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


def main():
    import torch
    px = VIEW.width * VIEW.height
    dv = torch.empty(px, dtype=torch.float64, device="cuda:0")
    dc = torch.empty(px, dtype=torch.int32, device="cuda:0")
    with MandelbrotDevice(0) as dev:
        for name, c in PARAMETERS.items():
            de, counts, st = dev.compute_julia_view_distance(VIEW, c, MRD)
            other, _, _ = dev.compute_julia_view_distance(VIEW, c, MRD, kernel="asm")
            assert np.array_equal(de, other)        # the two designs store the same values at the size that is timed
            esc = counts > 0
            legs = {"smooth": lambda: dev.launch_julia_view(VIEW, c, MRD, d_counts=dc.data_ptr(), d_smooth=dv.data_ptr()),
                    "distance_two_pass": lambda: dev.launch_julia_view_distance(VIEW, c, MRD, d_distance=dv.data_ptr(), d_counts=dc.data_ptr()),
                    "distance_one_pass": lambda: dev.launch_julia_view_distance(VIEW, c, MRD, d_distance=dv.data_ptr(), d_counts=dc.data_ptr(),
                                                                                kernel="asm"),
                    "smooth_asm": lambda: dev.launch_julia_view(VIEW, c, MRD, d_counts=dc.data_ptr(), d_smooth=dv.data_ptr(), kernel="asm")}
            ms = {}
            for _round in range(2):
                for leg, fn in legs.items():
                    ms.setdefault(leg, []).append(timed(torch, fn))
            for leg, v in ms.items():
                t = min(v)
                print(json.dumps({"c": name, "leg": leg, "ms": round(t, 4), "ms_runs": [round(x, 4) for x in v],
                                  "ratio_to_smooth": round(t / min(ms["smooth"]), 3),
                                  "ref_pixel_steps": int(st.pixel_iterations), "never_pixels": int(st.never_pixels),
                                  "escaped_pixel_steps": int(counts[esc].astype(np.int64).sum())}), flush=True)


if __name__ == "__main__":
    main()
