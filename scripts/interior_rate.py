#!/usr/bin/env python3
"""Interior-view measurements (profiles/interior/README.md).

    python scripts/interior_rate.py

BASELINE cfg2's and cfg5's view (the full set at 4096^2) at mrd 1000 and 4096, in one session: launch_view_interior (counts,
periods and distances), launch_view_distance with the default selector, and launch_view (the counts alone: pass 1 of both).
Device buffers, the null stream, HIP events around single launches, the median of 5 after 150 ms of untimed launches of the same
leg (the clock ramp of bench.py).  Prints one JSON line per mrd: the milliseconds, the share of count-0 pixels that settle, and
pass 2's share of the interior launch's time."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, View   # noqa: E402

VIEW = View(-2.0, -1.5, 3.0, 3.0, 4096, 4096)
RAMP_MS = 150.0


def timed(torch, fn):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < RAMP_MS:
        fn()
        torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def main():
    import torch
    px = VIEW.width * VIEW.height
    dv = torch.empty(px, dtype=torch.float64, device="cuda:0")
    dc = torch.empty(px, dtype=torch.int32, device="cuda:0")
    dp = torch.empty(px, dtype=torch.int32, device="cuda:0")
    with MandelbrotDevice(0) as dev:
        for mrd in (1000, 4096):
            legs = {"interior": lambda: dev.launch_view_interior(VIEW, mrd, d_period=dp.data_ptr(), d_distance=dv.data_ptr(), d_counts=dc.data_ptr()),
                    "distance": lambda: dev.launch_view_distance(VIEW, mrd, d_distance=dv.data_ptr(), d_counts=dc.data_ptr()),
                    "counts": lambda: dev.launch_view(VIEW, mrd, d_counts=dc.data_ptr())}
            out = {"view": "cfg2/cfg5 4096^2", "mrd": mrd}
            for leg, fn in legs.items():
                med, runs = timed(torch, fn)
                out[leg + "_ms"] = round(med, 4)
                out[leg + "_ms_runs"] = [round(x, 4) for x in runs]
            legs["interior"]()
            torch.cuda.synchronize()
            inside = int((dc == 0).sum().item())
            settled = int(((dc == 0) & (dp > 0)).sum().item())
            out.update(count0_pixels=inside, settled_pixels=settled, settled_share=round(settled / max(inside, 1), 4),
                       max_period=int(dp.max().item()),
                       pass2_share_of_interior=round(1.0 - out["counts_ms"] / out["interior_ms"], 4),
                       interior_to_distance=round(out["interior_ms"] / out["distance_ms"], 3))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
