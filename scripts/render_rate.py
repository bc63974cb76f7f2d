#!/usr/bin/env python3
"""Rendering measurements (profiles/render/README.md).

    python scripts/render_rate.py wall      render_view against compute_view_smooth into pinned memory (cfg5's view), and s = 2
    python scripts/render_rate.py kernels   4096^2 renders at s = 1, 2, 4, both sources -- run under
                                            `rocprofv3 --kernel-trace --stats -- python scripts/render_rate.py kernels` for
                                            the resolve kernel's own time

Legs alternate within one process and each lasts >= 50 ms after a warm-up, as bench.py does it."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, Palette, View   # noqa: E402
from distributedmandelbrot_amd import _lib as L   # noqa: E402

CFG5 = (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 5000)


def leg(fn, min_seconds=0.05, min_calls=3):
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= min_calls:
            return dt / n


def wall():
    view, mrd = CFG5
    pal = Palette.cosine()
    with MandelbrotDevice(0) as dev:
        lib, h = dev._lib, dev._h
        cv = dev._cview(view, None)
        rgba = dev.pinned_empty((4096, 4096, 4), np.uint8)
        nu = dev.pinned_empty((4096, 4096), np.float64)
        counts = dev.pinned_empty((4096, 4096), np.int32)

        def parent_nu():
            assert lib.mbk_view_compute_smooth(h, C.byref(cv), mrd, 0, None, nu.ctypes.data, None) == 0

        def parent_nu_counts():
            assert lib.mbk_view_compute_smooth(h, C.byref(cv), mrd, 0, counts.ctypes.data, nu.ctypes.data, None) == 0

        legs = {"compute_view_smooth_nu_pinned": parent_nu, "compute_view_smooth_nu_counts_pinned": parent_nu_counts,
                "render_view_s1": lambda: dev.render_view(view, mrd, palette=pal, out=rgba),
                "render_view_s2": lambda: dev.render_view(view, mrd, palette=pal, supersample=2, out=rgba)}
        for _ in range(3):   # clock ramp
            parent_nu()
        rounds = {k: [] for k in legs}
        for _ in range(5):
            for k, fn in legs.items():
                rounds[k].append(leg(fn) * 1e3)
        _, st1 = dev.render_view(view, mrd, palette=pal, out=rgba)
        _, st2 = dev.render_view(view, mrd, palette=pal, supersample=2, out=rgba)
        out = {k: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for k, v in rounds.items()}
        out["ratio_render_s1_over_parent_nu"] = out["render_view_s1"]["median_ms"] / out["compute_view_smooth_nu_pinned"]["median_ms"]
        out["ratio_s2_over_s1"] = out["render_view_s2"]["median_ms"] / out["render_view_s1"]["median_ms"]
        out["render_s1_stats"] = {"kernel_ms": st1.kernel_ms, "d2h_ms": st1.d2h_ms}
        out["render_s2_stats"] = {"kernel_ms": st2.kernel_ms, "d2h_ms": st2.d2h_ms}
        out["device"] = dev.info()["name"]
        out["pci"] = dev.pci_bus_id()
        print(json.dumps(out))


def kernels():
    view = View(-2.0, -1.5, 3.0, 3.0, 4096, 4096)
    mrd = 64   # the samples are cheap: this run is about the resolve kernel
    smooth, viewer = Palette.cosine(), Palette.viewer()
    with MandelbrotDevice(0) as dev:
        rgba = dev.pinned_empty((4096, 4096, 4), np.uint8)
        for s in (1, 2, 4):
            for source, pal in (("smooth", smooth), ("bytes", viewer)):
                for _ in range(6):
                    dev.render_view(view, mrd, palette=pal, source=source, supersample=s, out=rgba)
        print("done", dev.info()["name"], dev.pci_bus_id())


if __name__ == "__main__":
    {"wall": wall, "kernels": kernels}[sys.argv[1]]()
