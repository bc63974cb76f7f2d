#!/usr/bin/env python3
"""Rates of density views (include/mbk.h, "Density views") on one GPU, for both builds of the replay kernel.

    python scripts/density_rate.py [--size 4096] [--target 2048] [--reps 5] [--out FILE] [--compact-lib PATH]

Cases: cfg2's view (full set, size^2 samples, mrd 1000) into a target^2 table, and the same view at mrd 10 000 with
min_count = 100.  Variants: the library as built ("plain": one lane per sample in image order) and a second build of the same
sources with -DMBK_DENSITY_COMPACT=1 ("compact": the qualifying samples listed by count band, 64 to a wave), compiled into the
git-ignored build/ directory unless --compact-lib names one.  Every (variant, case) runs in a child process of its own under
its own time limit; the first failure ends the run.

Per run, from device events on one stream, the median of --reps after a clock ramp: the count pass alone (mbk_view_launch with
counts, the default selector -- the same launch the density call makes first), the whole density launch, and their
difference, the replay pass; deposits per second of the replay pass and of the whole launch; the ratio of the replay pass to
the count pass.  The table's crc32 is printed so that the variants can be compared.  Beside them the host twin's deposits per
second on a 512^2 view of the same rectangle (one CPU thread): what a caller without these calls has.
Prints one JSON line per run and a summary line; --out appends them to a file as well.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = {"cfg2_mrd1000": dict(mrd=1000, min_count=1), "cfg2_mrd10000_min100": dict(mrd=10000, min_count=100)}
RECT = (-2.0, -1.5, 3.0, 3.0)   # cfg2's view; the target is the same rectangle


def build_compact() -> str:
    from distributedmandelbrot_amd import build as B
    return B.build_variant("density_compact", B.VARIANTS["density_compact"])


def child(args) -> int:
    from distributedmandelbrot_amd import _lib as L
    if args.lib:
        L.SO_PATH = args.lib
    import numpy as np
    import torch
    from distributedmandelbrot_amd import DensityTarget, MandelbrotDevice, View
    case = CASES[args.case]
    mrd, lo = case["mrd"], case["min_count"]
    view = View(*RECT, args.size, args.size)
    target = DensityTarget(*RECT, args.target, args.target)
    with MandelbrotDevice(0) as dev:
        stream = torch.cuda.Stream()
        sid = stream.cuda_stream
        counts = torch.empty(args.size * args.size, dtype=torch.int32, device="cuda:0")
        table = torch.zeros(args.target * args.target, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def count_pass():
            dev.launch_view(view, mrd, d_counts=counts.data_ptr(), stream=sid)

        def density():
            dev.launch_view_density(view, target, mrd, d_density=table.data_ptr(), min_count=lo, stream=sid)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        with torch.cuda.stream(stream):
            t0 = time.time()
            while time.time() - t0 < 1.0:   # clock ramp, and both paths warm
                count_pass()
                stream.synchronize()
            density()
            stream.synchronize()
            table.zero_()
            stream.synchronize()
            tc, td = [], []
            for _ in range(args.reps):      # alternating, so that drift hits both alike
                tc.append(timed(count_pass))
                td.append(timed(density))
            mx, total = dev.density_max(table.data_ptr(), table.numel(), stream=sid)
            st = dev.reduce_counts(counts.data_ptr(), counts.numel(), mrd, stream=sid)
        host = table.cpu().numpy().view(np.uint32)
        assert total % args.reps == 0
        deposits = total // args.reps
        count_ms, density_ms = statistics.median(tc), statistics.median(td)
        replay_ms = density_ms - count_ms
        print(json.dumps({
            "variant": args.variant, "case": args.case, "size": args.size, "target": args.target, "mrd": mrd, "min_count": lo,
            "reps": args.reps, "count_ms": round(count_ms, 4), "density_ms": round(density_ms, 4), "replay_ms": round(replay_ms, 4),
            "count_ms_all": [round(x, 4) for x in tc], "density_ms_all": [round(x, 4) for x in td],
            "deposits": deposits, "max_cell_per_launch": mx // args.reps if mx % args.reps == 0 else mx / args.reps,
            "pixel_iterations": st.pixel_iterations, "never_pixels": st.never_pixels,
            "count_pass_G_pixel_iter_per_s": round(st.pixel_iterations / count_ms / 1e6, 1),
            "replay_G_deposits_per_s": round(deposits / replay_ms / 1e6, 3),
            "launch_G_deposits_per_s": round(deposits / density_ms / 1e6, 3),
            "replay_over_count": round(replay_ms / count_ms, 3),
            "table_crc32": zlib.crc32(host.tobytes()) & 0xffffffff,
            "device": dev.info()["name"]}), flush=True)
    return 0


def host_rate() -> dict:
    from distributedmandelbrot_amd import DensityTarget, View
    from distributedmandelbrot_amd.device import density_host
    out = {}
    for name, case in CASES.items():
        t0 = time.time()
        _, ds = density_host(View(*RECT, 512, 512), DensityTarget(*RECT, 256, 256), case["mrd"], min_count=case["min_count"])
        dt = time.time() - t0
        out[name] = {"host_seconds": round(dt, 3), "host_deposits": ds.deposits,
                     "host_M_deposits_per_s": round(ds.deposits / dt / 1e6, 2)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--target", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child run")
    ap.add_argument("--out", default="")
    ap.add_argument("--compact-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--variant", default="plain")
    ap.add_argument("--case", default="cfg2_mrd1000")
    args = ap.parse_args()
    if args.child:
        return child(args)

    lines = []

    def emit(obj) -> None:
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    from distributedmandelbrot_amd import build as B
    B.build()
    compact = args.compact_lib or build_compact()
    emit({"host_twin": host_rate()})
    results = {}
    for case in CASES:
        for variant, lib in (("plain", ""), ("compact", compact)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--variant", variant, "--case", case, "--size", str(args.size),
                   "--target", str(args.target), "--reps", str(args.reps)] + (["--lib", lib] if lib else [])
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                emit({"variant": variant, "case": case, "error": f"no result within {args.timeout} s"})
                return 1   # nothing more is started on the GPU after a run that hung
            if p.returncode != 0:
                emit({"variant": variant, "case": case, "error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]})
                return 1   # ... or failed
            results[(variant, case)] = json.loads(p.stdout.strip().splitlines()[-1])
            emit(results[(variant, case)])
    summary = {}
    for case in CASES:
        a, b = results[("plain", case)], results[("compact", case)]
        summary[case] = {"tables_identical": a["table_crc32"] == b["table_crc32"] and a["deposits"] == b["deposits"],
                         "plain_replay_ms": a["replay_ms"], "compact_replay_ms": b["replay_ms"],
                         "compact_over_plain": round(b["replay_ms"] / a["replay_ms"], 3)}
    emit({"summary": summary})
    return 0 if all(v["tables_identical"] for v in summary.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
