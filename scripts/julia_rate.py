#!/usr/bin/env python
"""GPU: kernel time of Julia views (mbk_julia_view_launch) -- 4096^2 at mrd 1000 for five parameters, three paths each --
beside the strict Mandelbrot loop on BASELINE cfg2 as the yardstick (the same arithmetic, the same loops).

    python scripts/julia_rate.py [out.json]

Per leg: launches back to back on one stream into device buffers between a pair of HIP events, as many as fill >= 50 ms
(sized from a probe launch), after a ramp of >= 300 ms of the same launch; five legs, the median.  Reported per launch:
kernel ms; reference pixel-iterations/s (what the contract's loop would run: n per escaped pixel, mrd - 1 per other, over the
time); executed pixel-iterations/s, the steps the lanes ran over the time, where that is KNOWN: the per-step loop runs exactly
the reference's steps.  The grouped loop runs each escaping lane on to the end of its group and replays it, and the cycle test
retires lanes early; the kernels keep no step counter, so no executed figure is given for those two paths (null) rather than a
guessed one.  Results and the raw output: profiles/julia/.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from distributedmandelbrot_amd import MandelbrotDevice, View  # noqa: E402

N, MRD = 4096, 1000
# (-0.8+0.156i lies outside the Mandelbrot set and i is a dendrite: neither has an interior, and -1 takes the literal loop.
# Douady's rabbit is the one here whose large interior runs through the grouped loop and the cycle test.  -1 and 1.5+1.5i
# take the per-step kernel on every selector, so all three of their figures are executed figures.)
PARAMS = [("-0.8+0.156i", (-0.8, 0.156)), ("-1", (-1.0, 0.0)), ("i", (0.0, 1.0)), ("1.5+1.5i", (1.5, 1.5)),
          ("-0.123+0.745i", (-0.123, 0.745))]
JULIA_VIEW = View(-1.6, -1.6, 3.2, 3.2, N, N)
CFG2 = View(-2.0, -1.5, 3.0, 3.0, N, N)
LEG_MS, RAMP_MS, LEGS = 50.0, 300.0, 5


def timed(launch):
    """Median ms per launch over LEGS legs of >= LEG_MS each, after a ramp."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def leg(reps):
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    one = max(leg(1), leg(2), 1e-3)
    leg(max(1, int(RAMP_MS / one) + 1))
    reps = max(3, int(LEG_MS / one) + 1)
    return statistics.median(leg(reps) for _ in range(LEGS)), reps


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = []
    with MandelbrotDevice(0) as dev:
        info = dev.info()
        d_counts = torch.empty(N * N, dtype=torch.int32, device="cuda:0")
        ptr = d_counts.data_ptr()
        cycle_default = dev.get_option("cycle_detect")

        def record(name, path, launch, ref_iters, executed_known):
            # executed_known: this launch runs the per-step kernel, whose lanes run exactly the reference's steps
            ms, reps = timed(launch)
            row = {"what": name, "path": path, "kernel_ms": round(ms, 4), "launches_per_leg": reps,
                   "reference_Gpi_per_s": round(ref_iters / ms / 1e6, 1),
                   "executed_Gpi_per_s": round(ref_iters / ms / 1e6, 1) if executed_known else None}
            rows.append(row)
            print(json.dumps(row), flush=True)

        # the yardstick: the strict Mandelbrot loop (MBK_KERNEL_ASM: every iteration executed) on cfg2, and the library's
        # default on the same view for scale
        ref = dev.compute_view(CFG2, MRD, want_bytes=False)[2].pixel_iterations
        record("mandelbrot cfg2", "asm", lambda: dev.launch_view(CFG2, MRD, d_counts=ptr, kernel="asm"), ref, True)
        record("mandelbrot cfg2", "default", lambda: dev.launch_view(CFG2, MRD, d_counts=ptr), ref, False)
        for name, c in PARAMS:
            st = dev.compute_julia_view(JULIA_VIEW, c, MRD, want_bytes=False)[3]
            ref = st.pixel_iterations
            per_step = abs(c[1]) < 2.0 ** -900 or c[0] * c[0] + c[1] * c[1] >= 4.0 - 1e-9   # the library's two rules (mbk.h)
            print(json.dumps({"what": f"julia {name}", "never_share": round(st.never_pixels / (N * N), 4),
                              "reference_pixel_iterations": ref}), flush=True)
            record(f"julia {name}", "asm", lambda: dev.launch_julia_view(JULIA_VIEW, c, MRD, d_counts=ptr, kernel="asm"), ref, True)
            dev.set_option("cycle_detect", 1)
            record(f"julia {name}", "default, cycle test", lambda: dev.launch_julia_view(JULIA_VIEW, c, MRD, d_counts=ptr), ref, per_step)
            dev.set_option("cycle_detect", 0)
            record(f"julia {name}", "default, no cycle test", lambda: dev.launch_julia_view(JULIA_VIEW, c, MRD, d_counts=ptr), ref, per_step)
            dev.set_option("cycle_detect", cycle_default)
        torch.cuda.synchronize()
    result = {"device": info["name"], "arch": info["arch"], "compute_units": info["compute_units"], "view": [N, N], "mrd": MRD,
              "leg_ms": LEG_MS, "ramp_ms": RAMP_MS, "legs": LEGS, "rows": rows}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"device": info["name"], "rows": len(rows)}))


if __name__ == "__main__":
    main()
