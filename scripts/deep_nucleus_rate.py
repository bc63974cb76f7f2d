"""Atom periods and Newton seeds (mbk_deep_view_launch_nucleus) beside the distance kernel whose loop they share
(mbk_deep_view_launch_distance), on the three views of scripts/deep_rate.py: 4096^2, mrd 30 000, spans 1e-8 and 1e-20 (seahorse
valley) and 1e-60 (c = i).  Kernel time from HIP events on one stream, median of `reps`, the two kernels alternating after a
clock ramp of ~2 s of the distance kernel.  Then the wall time of a full MandelbrotDevice.locate_nucleus -- kernel, download,
pick_nucleus_seed, refine_nucleus -- on the three 16 x 16 cases of tests/test_deep_nucleus.py and on 256 x 256 views of the
same spans, with its parts.
    python scripts/deep_nucleus_rate.py [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decimal import Decimal, getcontext
import numpy as np
import torch
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, NucleusError, pick_nucleus_seed
from distributedmandelbrot_amd.device import _exact_fraction, nucleus_precision_bits, refine_nucleus

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mrd, n = 30000, 4096
dev = MandelbrotDevice(0)
d_counts = torch.empty(n * n, dtype=torch.int32, device="cuda:0")
d_period = torch.empty(n * n, dtype=torch.int32, device="cuda:0")
d_val = torch.empty(2 * n * n, dtype=torch.float64, device="cuda:0")
stream = torch.cuda.Stream(device="cuda:0")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


for centre, span in ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60)):
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, n)
    dist = lambda: dev.launch_deep_view_distance(orbit, view, mrd, d_rel=d_val.data_ptr(), d_counts=d_counts.data_ptr(), stream=stream.cuda_stream)
    nucl = lambda: dev.launch_deep_view_nucleus(orbit, view, mrd, d_period=d_period.data_ptr(), d_delta=d_val.data_ptr(),
                                                d_counts=d_counts.data_ptr(), stream=stream.cuda_stream)
    dist()
    nucl()           # upload + warm-up of both
    stream.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:          # the clock ramp
        timed(dist)
    a, b = [], []
    for _ in range(reps):
        a.append(timed(dist))
        b.append(timed(nucl))
    counts = d_counts.cpu().numpy().astype(np.int64)
    steps = np.where(counts > 0, counts, mrd - 1)
    periods = d_period.cpu().numpy()
    ka, kb = float(np.median(a)), float(np.median(b))
    print(f"span {span:g} P {orbit.precision_bits} M {orbit.length}: distance {ka:.2f} ms (min {min(a):.2f}), nucleus {kb:.2f} ms "
          f"(min {min(b):.2f}), ratio {kb / ka:.3f}; pixel-steps {int(steps.sum()):,} = {steps.sum() / (kb * 1e-3) / 1e12:.3f} T/s; "
          f"periods {int(periods.min())} .. {int(periods.max())}", flush=True)


def misiurewicz():
    getcontext().prec = 1320
    c = Decimal("-1.5436890126920763615708559718")
    for _ in range(12):
        c = c - (((c + 2) * c + 2) * c + 2) / ((3 * c + 4) * c + 2)
    return str(c.quantize(Decimal(10) ** -1300))


for name, centre, span, lmrd in (("i-1e-20", ("0", "1"), 1e-20, 1500), ("i-1e-200", ("0", "1"), 1e-200, 4000),
                                 ("mis-1e-100", (misiurewicz(), "0"), 1e-100, 3000)):
    orbit = DeepOrbit(*centre, lmrd, min_span=span)
    for w in (16, 256):
        view = DeepView(span, w)
        try:
            dev.locate_nucleus(orbit, view, lmrd)      # warm-up (the orbit's upload)
        except NucleusError as err:
            print(f"locate {name} {w} x {w}: {err}", flush=True)
            continue
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            nuc = dev.locate_nucleus(orbit, view, lmrd)
            walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        period, delta, _, st = dev.compute_deep_view_nucleus(orbit, view, lmrd)
        t1 = time.perf_counter()
        seed = pick_nucleus_seed(view, period, delta)
        t2 = time.perf_counter()
        C0 = (_exact_fraction(orbit.center[0]), _exact_fraction(orbit.center[1]))
        refine_nucleus(C0[0] + seed.offset_r, C0[1] + seed.offset_i, seed.period, nucleus_precision_bits(view))
        t3 = time.perf_counter()
        print(f"locate {name} {w} x {w}: wall {np.median(walls) * 1e3:.1f} ms (min {min(walls) * 1e3:.1f}) = compute "
              f"{(t1 - t0) * 1e3:.1f} (kernel {st.kernel_ms:.2f}) + pick {(t2 - t1) * 1e3:.1f} + refine {(t3 - t2) * 1e3:.1f} ms; period "
              f"{nuc.period}, {nuc.rounds} rounds at {nuc.precision_bits} bits + {nuc.polish_rounds} polishing, |size| 2^{nuc.size_log2:.1f}, inside {nuc.inside}", flush=True)
dev.close()
