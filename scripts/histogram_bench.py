#!/usr/bin/env python3
"""Histogram measurements (profiles/histogram/README.md).

    python scripts/histogram_bench.py kernels   mbk_counts_histogram against mbk_reduce_counts (the existing kernel that streams
                                                the same bytes) on 4096^2 and 8192^2 count buffers: cfg2's counts, one value,
                                                uniformly random counts at mrd 30 000 and 2^20.  Wall time per call, each call
                                                followed by a synchronise (mbk_reduce_counts ends in one), and the device-side
                                                time of 20 histogram launches back to back between two events.
    python scripts/histogram_bench.py wall      render_view(source="equalized") beside source="smooth" and view_histogram, cfg5's view
    python scripts/histogram_bench.py trace     the dispatches of `kernels` (20 of each per input) and one equalized render, to
                                                run under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`
    python scripts/histogram_bench.py summarise DIR   per-input kernel times from that run's *_kernel_trace.csv

Legs alternate within one process and each lasts >= 50 ms after a clock ramp and a warm-up call, as bench.py does it."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, Palette, View   # noqa: E402

CFG2 = (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 1000)
CFG5 = (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 5000)
TRACE_CALLS = 20


def leg(fn, min_seconds=0.05, min_calls=3):
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= min_calls:
            return dt / n


def inputs(dev, torch):
    """(name, mrd, device int32 tensor) for both sizes.  cfg2's counts at 8192^2 are the same view at twice the resolution."""
    rs = np.random.RandomState(5)
    for side in (4096, 8192):
        n = side * side
        view = View(-2.0, -1.5, 3.0, 3.0, side, side)
        t = torch.empty(n, dtype=torch.int32, device="cuda:0")
        dev.launch_view(view, CFG2[1], d_counts=t.data_ptr())
        torch.cuda.synchronize()
        yield f"cfg2 counts {side}^2", CFG2[1], t
        yield f"one value (12345) {side}^2", 30000, torch.full((n,), 12345, dtype=torch.int32, device="cuda:0")
        yield f"one value (0) {side}^2", 30000, torch.zeros(n, dtype=torch.int32, device="cuda:0")
        yield f"random mrd 30000 {side}^2", 30000, torch.from_numpy(rs.randint(0, 30000, n).astype(np.int32)).to("cuda:0")
        yield f"random mrd 2^20 {side}^2", 1 << 20, torch.from_numpy(rs.randint(0, 1 << 20, n).astype(np.int32)).to("cuda:0")


def kernels():
    import torch
    with MandelbrotDevice(0) as dev:
        out = {"device": dev.info()["name"], "cus": dev.info()["compute_units"], "pci": dev.pci_bus_id(), "inputs": {}}
        hist = torch.zeros(1 << 20, dtype=torch.int64, device="cuda:0")
        ramp = torch.zeros(1 << 24, dtype=torch.int32, device="cuda:0")
        for _ in range(200):   # clock ramp
            dev.reduce_counts(ramp.data_ptr(), ramp.numel(), 1000)
        for name, mrd, t in inputs(dev, torch):
            n = t.numel()

            def histogram():
                dev.counts_histogram(t.data_ptr(), n, mrd, hist.data_ptr())
                torch.cuda.synchronize()

            def reduce():
                dev.reduce_counts(t.data_ptr(), n, mrd)

            hist.zero_()
            rounds = {"histogram": [], "reduce": []}
            for _ in range(3):
                rounds["histogram"].append(leg(histogram) * 1e6)
                rounds["reduce"].append(leg(reduce) * 1e6)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(TRACE_CALLS):
                dev.counts_histogram(t.data_ptr(), n, mrd, hist.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            h, r = float(np.median(rounds["histogram"])), float(np.median(rounds["reduce"]))
            out["inputs"][name] = {"histogram_wall_us": h, "reduce_wall_us": r, "ratio": h / r,
                                   "histogram_back_to_back_us": e0.elapsed_time(e1) * 1e3 / TRACE_CALLS,
                                   "bytes": 4 * n, "rounds": rounds}
            del t
        print(json.dumps(out))


def wall():
    view, mrd = CFG5
    smooth = Palette.cosine()
    eq = Palette.cosine().for_equalized()
    with MandelbrotDevice(0) as dev:
        rgba = dev.pinned_empty((4096, 4096, 4), np.uint8)
        legs = {"render_view_smooth_s1": lambda: dev.render_view(view, mrd, palette=smooth, out=rgba),
                "render_view_equalized_s1": lambda: dev.render_view(view, mrd, palette=eq, source="equalized", out=rgba),
                "view_histogram": lambda: dev.view_histogram(view, mrd),
                "compute_view_counts_unpinned": lambda: dev.compute_view(view, mrd, want_bytes=False)}
        lut = None
        for _ in range(3):   # clock ramp
            dev.render_view(view, mrd, palette=smooth, out=rgba)
        rounds = {k: [] for k in legs}
        for _ in range(5):
            for k, fn in legs.items():
                rounds[k].append(leg(fn) * 1e3)
        from distributedmandelbrot_amd.image import equalize_lut
        hist, hst = dev.view_histogram(view, mrd, want_stats=True)
        lut = equalize_lut(hist)
        rounds["render_view_equalized_s1_given_lut"] = [
            leg(lambda: dev.render_view(view, mrd, palette=eq, source="equalized", out=rgba, lut=lut)) * 1e3 for _ in range(5)]
        t0 = time.perf_counter()
        for _ in range(20):
            equalize_lut(hist)
        out = {k: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for k, v in rounds.items()}
        out["equalize_lut_host_ms"] = (time.perf_counter() - t0) / 20 * 1e3
        out["ratio_equalized_over_smooth"] = out["render_view_equalized_s1"]["median_ms"] / out["render_view_smooth_s1"]["median_ms"]
        out["view_histogram_stats"] = {"kernel_ms": hst.kernel_ms, "d2h_ms": hst.d2h_ms}
        out["device"] = dev.info()["name"]
        out["pci"] = dev.pci_bus_id()
        print(json.dumps(out))


def trace():
    import torch
    with MandelbrotDevice(0) as dev:
        hist = torch.zeros(1 << 20, dtype=torch.int64, device="cuda:0")
        for name, mrd, t in inputs(dev, torch):
            for _ in range(TRACE_CALLS):
                dev.counts_histogram(t.data_ptr(), t.numel(), mrd, hist.data_ptr())
            torch.cuda.synchronize()
            for _ in range(TRACE_CALLS):
                dev.reduce_counts(t.data_ptr(), t.numel(), mrd)
            print("traced", name)
            del t
        view, mrd = CFG5
        rgba = dev.pinned_empty((4096, 4096, 4), np.uint8)
        dev.render_view(view, mrd, palette=Palette.cosine().for_equalized(), source="equalized", out=rgba)
        print("done", dev.info()["name"], dev.pci_bus_id())


def summarise(directory):
    """Median kernel time of each run of TRACE_CALLS equal dispatches of the two kernels, in dispatch order (= inputs() order)."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    groups = []
    for start, end, name in rows:
        kind = "histogram" if "counts_histogram_kernel" in name else ("reduce" if "reduce_vec_kernel" in name else None)
        if kind is None:
            continue
        if not groups or groups[-1][0] != kind or len(groups[-1][1]) == TRACE_CALLS:
            groups.append((kind, []))
        groups[-1][1].append((end - start) / 1e3)
    print(json.dumps([{"kernel": k, "calls": len(v), "median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}
                      for k, v in groups]))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "summarise":
        summarise(sys.argv[2])
    else:
        {"kernels": kernels, "wall": wall, "trace": trace}[mode]()
