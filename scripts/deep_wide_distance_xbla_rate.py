"""Distance estimates for extended-range deep views with bilinear approximation: kernel time of
deep_wide_distance_bla_kernel (launch_wide_view_distance_xbla) beside the full-step deep_wide_distance_kernel
(launch_wide_view_distance) and the count-only deep_wide_bla_kernel (launch_deep_view, xbla) on the same WideDeepView in the
same run.  The view is that of scripts/deep_wide_distance_rate.py -- c = i at range 1, exp2 = -1100, n x n, mrd 3000 -- and
after it one where few steps skip: the seahorse-valley centre at span 1e-8 written as a wide view (n2 x n2, mrd 30 000).  All
launches go to one torch stream between HIP events; the first call of the new launch (it builds and uploads the table) is paid
and reported before anything is timed; a clock ramp of `ramp` untimed launches of each comes next, then `legs` legs in which the
three alternate, `reps` launches each per leg; the figure of a kernel is the median over all its timed launches, and the spread
over the legs' medians is printed beside it.  The steps-executed share is a host figure (tests/test_deep_wide_distance_bla.py
prints it per case).   python scripts/deep_wide_distance_xbla_rate.py [n] [legs] [reps] [ramp] [n2]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, WideDeepView

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 6144
legs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ramp = int(sys.argv[4]) if len(sys.argv) > 4 else 3
n2 = int(sys.argv[5]) if len(sys.argv) > 5 else 4096
dev = MandelbrotDevice(0)
stream = torch.cuda.Stream(device="cuda:0")


def timed(launch) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    launch()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


def run(centre, view, mrd, what):
    px = view.width * view.height
    orbit = DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)
    fc, xc, cc = (torch.zeros(px, dtype=torch.int32, device="cuda:0") for _ in range(3))
    frel, xrel = (torch.zeros(px, dtype=torch.float64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    launches = {
        "full-step distance": lambda: dev.launch_wide_view_distance(orbit, view, mrd, d_rel=frel.data_ptr(), d_counts=fc.data_ptr(),
                                                                    stream=stream.cuda_stream),
        "xbla distance": lambda: dev.launch_wide_view_distance_xbla(orbit, view, mrd, d_rel=xrel.data_ptr(), d_counts=xc.data_ptr(),
                                                                    stream=stream.cuda_stream),
        "xbla counts only": lambda: dev.launch_deep_view(orbit, view, mrd, d_counts=cc.data_ptr(), stream=stream.cuda_stream, xbla=True),
    }
    t0 = time.perf_counter()
    launches["xbla distance"]()          # the first call: the wide orbit's upload, the table built on the host and uploaded
    stream.synchronize()
    t_first = time.perf_counter() - t0
    for _ in range(ramp):
        for launch in launches.values():
            timed(launch)
    ms = {name: [] for name in launches}
    for _ in range(legs):
        for name, launch in launches.items():
            ms[name].append([timed(launch) for _ in range(reps)])
    f, x, c = fc.cpu().numpy(), xc.cpu().numpy(), cc.cpu().numpy()
    assert np.array_equal(x, c)          # the count is exactly the MBK_DEEP_XBLA count
    fr, xr = frel.cpu().numpy(), xrel.cpu().numpy()
    steps = int(np.where(f > 0, f, mrd - 1).astype(np.int64).sum())
    both = (f > 0) & (x == f) & np.isfinite(fr) & (fr > 0)
    err = np.abs(xr[both] - fr[both]) / fr[both]
    print(f"{torch.cuda.get_device_name(0)}: {what}, {view.width} x {view.height}, mrd {mrd}, P {orbit.precision_bits}, M {orbit.length}: "
          f"{steps:,} counted pixel-steps of the full-step launch, {int((f == 0).sum())} never escaped; first xbla distance call "
          f"(table) {t_first * 1e3:.1f} ms; counts equal the full-step launch's on {float((x == f).mean()) * 100:.4f} % of pixels; "
          f"xbla rel finite and > 0 on {float((np.isfinite(xr) & (xr > 0))[x > 0].mean()) * 100:.4f} % of escaped pixels; "
          f"|xbla rel - full rel| / full rel where the counts agree: median {np.median(err):.2e}, 99.9 % {np.quantile(err, 0.999):.2e}, "
          f"max {err.max():.2e}")
    med, span = {}, {}
    for name, rows in ms.items():
        a = np.array(rows)
        med[name] = float(np.median(a))
        per_leg = np.median(a, axis=1)
        span[name] = (float(per_leg.min()), float(per_leg.max()))
        print(f"  {name}: kernel ms median {med[name]:.2f} over {a.size} launches (min {a.min():.2f}, max {a.max():.2f}; legs' medians "
              f"{per_leg.min():.2f} .. {per_leg.max():.2f})")
    print(f"  xbla distance / full-step distance: {med['xbla distance'] / med['full-step distance']:.4f}; "
          f"xbla distance / xbla counts only: {med['xbla distance'] / med['xbla counts only']:.3f}; the legs are "
          f"{'apart' if span['xbla distance'][1] < span['full-step distance'][0] else 'NOT apart'}", flush=True)


run(("0", "1"), WideDeepView(1.0, -1100, n), 3000, "c = i, range 1, exp2 -1100")
e = math.frexp(1e-8)[1] - 2                          # the range in [2, 4)
run(SEAHORSE, WideDeepView(math.ldexp(1e-8, -e), e, n2), 30000, "seahorse centre, span 1e-8 as a wide view")
dev.close()
