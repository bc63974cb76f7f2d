"""Extended-range deep views with bilinear approximation (MBK_DEEP_XBLA): kernel time of deep_wide_bla_kernel beside
deep_wide_kernel on the same view in the same run -- the two alternate after a warm-up of each, so both see the same clocks;
kernel time from HIP events, median of `reps` -- and the share of pixels whose counts are equal.  The view the feature is for
is c = i at range 1, exp2 = -1100 (4096^2, mrd 30 000), a span no plain view can name; after it the three views of
scripts/deep_wide_rate.py (spans 1e-8 and 1e-20 at the seahorse-valley centre, 1e-60 at c = i) written as wide views.  The
statistics count the reference's iterations, not the steps executed: the executed share is a host figure
(tests/test_deep_wide_bla.py prints it per case).   python scripts/deep_wide_bla_rate.py [reps] [n]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, WideDeepView

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
mrd = 30000
dev = MandelbrotDevice(0)
wcounts = dev.pinned_empty((n, n), np.int32)
xcounts = dev.pinned_empty((n, n), np.int32)


def timed(orbit, view, out, xbla):
    return dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=out, xbla=xbla)[3]


def line(what, ks, st, out):
    k = float(np.median(ks))
    return (f"  {what}: kernel ms median {k:.2f} (min {min(ks):.2f}); reference pixel-iterations {st.pixel_iterations:,} = "
            f"{st.pixel_iterations / (k * 1e-3) / 1e12:.3f} T/s; never escaped {st.never_pixels}; distinct counts {len(np.unique(out))}")


def run(centre, view, what):
    t0 = time.perf_counter()
    orbit = DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)
    t_orbit = time.perf_counter() - t0
    timed(orbit, view, wcounts, False)               # uploads + warm-up
    t0 = time.perf_counter()
    timed(orbit, view, xcounts, True)                # ... and the table: built on the host, uploaded
    t_first = time.perf_counter() - t0
    kw, kx = [], []
    for _ in range(reps):
        sw = timed(orbit, view, wcounts, False)
        sx = timed(orbit, view, xcounts, True)
        kw.append(sw.kernel_ms)
        kx.append(sx.kernel_ms)
    print(f"{what} centre ({centre[0][:12]}, {centre[1][:12]}) {n} x {n} mrd {mrd} P {orbit.precision_bits} M {orbit.length}: "
          f"orbit {t_orbit * 1e3:.1f} ms host, first xbla call (table) {t_first * 1e3:.1f} ms; xbla / wide "
          f"{np.median(kx) / np.median(kw):.3f}; counts equal on {float((wcounts == xcounts).mean()) * 100:.4f} % of pixels")
    print(line("wide", kw, sw, wcounts))
    print(line("xbla", kx, sx, xcounts), flush=True)


run(("0", "1"), WideDeepView(1.0, -1100, n), "range 1, exp2 -1100 (span 2^-1100 ~ 1e-331)")
for centre, span in ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60)):
    e = math.frexp(span)[1] - 2                      # the range in [2, 4)
    run(centre, WideDeepView(math.ldexp(span, -e), e, n), f"span {span:g}")
dev.close()
