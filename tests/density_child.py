#!/usr/bin/env python3
"""Every case of tests/density_cases.py, and the two band-loop views, on one MandelbrotDevice of a library named on the
command line -- a second build of the sources, such as the compact replay's (build.build_variant) -- with the results in one
.npz for the parent to compare with the model.  A process keeps one library (_lib.load), hence a process of its own:

    python tests/density_child.py --lib PATH --out FILE

Not a test module.  Exit status 0: every case ran (whether its numbers are right is for the parent to say).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from distributedmandelbrot_amd import _lib as L
    L.SO_PATH = os.path.abspath(args.lib)   # before anything loads
    import numpy as np
    from distributedmandelbrot_amd import MandelbrotDevice
    import density_cases as DC
    lib = L.load()
    assert lib._name == L.SO_PATH, lib._name
    compact = int(lib.mbk_density_build_info())
    out = {"build_info": np.int64(compact)}
    t0 = time.time()
    with MandelbrotDevice(0) as dev:
        for case in DC.CASES:
            for key, value in DC.run_case(dev, case).items():
                out[f"{case.name}__{key}"] = np.asarray(value)
        out["cases_seconds"] = np.float64(time.time() - t0)
        print(f"{len(DC.CASES)} cases in {time.time() - t0:.2f} s (MBK_DENSITY_COMPACT = {compact})", flush=True)
        for name, view, windows in DC.band_views(8 if compact else 4, L.MBK_RENDER_BAND_BYTES):
            t1 = time.time()
            for key, value in DC.run_band_view(dev, view, windows).items():
                out[f"band_{name}__{key}"] = np.asarray(value)
            out[f"band_{name}__seconds"] = np.float64(time.time() - t1)
            print(f"band view {name} {view.width} x {view.height} in {time.time() - t1:.2f} s", flush=True)
    np.savez(args.out, **out)
    print(f"child done in {time.time() - t0:.2f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
