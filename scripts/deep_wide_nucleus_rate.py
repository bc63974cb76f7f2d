"""Atom periods and Newton seeds of extended-range deep views (mbk_deep_xview_launch_nucleus) beside the wide distance kernel
whose loop they share (mbk_deep_xview_launch_distance), on the same views: c = i and the Misiurewicz point of
tests/test_deep_wide.py at span 2^-1100, 4096^2, mrd 3000, and the view Nucleus.view frames around the period-534 minibrot found
at c = i, span 1e-200 (about 2^-1330 wide, mrd 2136).  Kernel time from HIP events on one stream, median of `reps`, the two
kernels alternating after a clock ramp of ~2 s of the distance kernel.  Then the wall time of a full
MandelbrotDevice.locate_wide_nucleus -- kernel, download, pick_wide_nucleus_seed, refine_nucleus -- on the two 16 x 16 cases of
tests/test_deep_wide_nucleus.py and on 256 x 256 views of the same spans, split into the device pass and the host refinement.
    python scripts/deep_wide_nucleus_rate.py [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decimal import Decimal, getcontext
import numpy as np
import torch
from distributedmandelbrot_amd import (DeepOrbit, DeepView, MandelbrotDevice, NucleusError, WideDeepView, pick_wide_nucleus_seed,
                                       wide_nucleus_precision_bits)
from distributedmandelbrot_amd.device import _exact_fraction, refine_nucleus


def misiurewicz():
    getcontext().prec = 1320
    c = Decimal("-1.5436890126920763615708559718")
    for _ in range(12):
        c = c - (((c + 2) * c + 2) * c + 2) / ((3 * c + 4) * c + 2)
    return str(c.quantize(Decimal(10) ** -1300))


CENTRES = (("c = i", ("0", "1")), ("Misiurewicz", (misiurewicz(), "0")))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mrd, n, exp2 = 3000, 4096, -1100
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


def views():
    for name, centre in CENTRES:
        view = WideDeepView(1.0, exp2, n)
        yield f"{name}, span 2^{exp2}", DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2), view, mrd
    # a view of another kind: the minibrot of period 534 that locate_nucleus finds at c = i, span 1e-200, framed by Nucleus.view
    # (4 sizes wide, about 2^-1330): its reference orbit is periodic, not parked on a repelling cycle
    first = dev.locate_nucleus(DeepOrbit("0", "1", 4000, min_span=1e-200), DeepView(1e-200, 16), 4000)
    yield f"minibrot of period {first.period}, span 2^{first.size_log2 + 2:.1f}", first.orbit(4 * first.period), first.view(n), 4 * first.period


for name, orbit, view, mrd in views():
    dist = lambda: dev.launch_wide_view_distance(orbit, view, mrd, d_rel=d_val.data_ptr(), d_counts=d_counts.data_ptr(), stream=stream.cuda_stream)
    nucl = lambda: dev.launch_wide_view_nucleus(orbit, view, mrd, d_period=d_period.data_ptr(), d_delta=d_val.data_ptr(),
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
    print(f"{name}, {n}^2, mrd {mrd}, P {orbit.precision_bits} M {orbit.length}: distance {ka:.2f} ms (min {min(a):.2f}), "
          f"nucleus {kb:.2f} ms (min {min(b):.2f}), ratio {kb / ka:.3f}; pixel-steps {int(steps.sum()):,} = "
          f"{steps.sum() / (kb * 1e-3) / 1e12:.3f} T/s; never escaped {int((counts == 0).sum())}; periods {int(periods.min())} .. "
          f"{int(periods.max())}", flush=True)

for name, centre in CENTRES:
    lmrd = 1600
    for w in (16, 256):
        view = WideDeepView(1.0, exp2, w)
        orbit = DeepOrbit(*centre, lmrd, min_span_exp2=view.min_span_exp2)
        try:
            dev.locate_wide_nucleus(orbit, view, lmrd)      # warm-up (the orbit's upload)
        except NucleusError as err:
            print(f"locate {name} {w} x {w}: {err}", flush=True)
            continue
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            nuc = dev.locate_wide_nucleus(orbit, view, lmrd)
            walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        period, delta, _, st = dev.compute_wide_view_nucleus(orbit, view, lmrd)
        t1 = time.perf_counter()
        seed = pick_wide_nucleus_seed(view, period, delta)
        t2 = time.perf_counter()
        C0 = (_exact_fraction(orbit.center[0]), _exact_fraction(orbit.center[1]))
        P = wide_nucleus_precision_bits(view)
        refine_nucleus(C0[0] + seed.offset_r, C0[1] + seed.offset_i, seed.period, P, max(32, -(-P // 40)))
        t3 = time.perf_counter()
        print(f"locate {name} 2^{exp2} {w} x {w}: wall {np.median(walls) * 1e3:.1f} ms (min {min(walls) * 1e3:.1f}) = device pass "
              f"{(t1 - t0) * 1e3:.1f} (kernel {st.kernel_ms:.2f}) + pick {(t2 - t1) * 1e3:.1f} + host refinement {(t3 - t2) * 1e3:.1f} ms; "
              f"period {nuc.period}, {nuc.rounds} rounds at {nuc.precision_bits} bits + {nuc.polish_rounds} polishing, "
              f"|size| 2^{nuc.size_log2:.1f}, seed pixel {nuc.seed_pixel}, inside {nuc.inside}", flush=True)
dev.close()
