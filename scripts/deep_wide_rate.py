"""Extended-range deep views (mbk_deep_xview_*): kernel time and executed pixel-steps/s of the wide kernel on the three 4096^2
views of scripts/deep_rate.py (mrd 30 000; spans 1e-8 and 1e-20 at the seahorse-valley centre, 1e-60 at c = i), written as
wide views of the same spans, beside the plain kernel on the same view in the same run (the two alternate, so both see the
same clocks; their counts are compared); and on one view no plain view can name, c = i at exp2 = -1100.  Every pixel runs
count (or mrd - 1) steps, so the executed steps are the stats' pixel_iterations.   python scripts/deep_wide_rate.py [reps]"""
import math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, WideDeepView

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mrd, n = 30000, 4096
dev = MandelbrotDevice(0)
counts = dev.pinned_empty((n, n), np.int32)
wcounts = dev.pinned_empty((n, n), np.int32)


def timed(orbit, view, out):
    t0 = time.perf_counter()
    _, _, _, st = dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=out)
    return st, time.perf_counter() - t0


def line(what, ks, st, out):
    k = float(np.median(ks))
    return (f"  {what}: kernel ms median {k:.2f} (min {min(ks):.2f}); pixel-steps {st.pixel_iterations:,} = "
            f"{st.pixel_iterations / (k * 1e-3) / 1e12:.3f} T/s; never escaped {st.never_pixels}; distinct counts {len(np.unique(out))}")


for centre, span in ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60)):
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    e = math.frexp(span)[1] - 2                      # the range in [2, 4)
    plain, wide = DeepView(span, n), WideDeepView(math.ldexp(span, -e), e, n)
    timed(orbit, plain, counts)                      # uploads + warm-up
    timed(orbit, wide, wcounts)
    kp, kw = [], []
    for _ in range(reps):
        sp, _ = timed(orbit, plain, counts)
        sw, _ = timed(orbit, wide, wcounts)
        kp.append(sp.kernel_ms)
        kw.append(sw.kernel_ms)
    print(f"span {span:g} centre ({centre[0][:12]}, {centre[1][:12]}) P {orbit.precision_bits} M {orbit.length}: "
          f"wide / plain {np.median(kw) / np.median(kp):.3f}; counts equal on {float((counts == wcounts).mean()) * 100:.4f} % of pixels")
    print(line("plain", kp, sp, counts))
    print(line("wide ", kw, sw, wcounts), flush=True)

exp2 = -1100
view = WideDeepView(1.0, exp2, n)
t0 = time.perf_counter()
orbit = DeepOrbit("0", "1", mrd, min_span_exp2=view.min_span_exp2)
t_orbit = time.perf_counter() - t0
timed(orbit, view, wcounts)
kw = [timed(orbit, view, wcounts)[0].kernel_ms for _ in range(reps)]
sw, _ = timed(orbit, view, wcounts)
print(f"range 1, exp2 {exp2} (span 2^{exp2} ~ 1e{exp2 * math.log10(2.0):.0f}, below binary64's range) centre (0, 1) "
      f"P {orbit.precision_bits} M {orbit.length}: orbit {t_orbit * 1e3:.1f} ms host")
print(line("wide ", kw, sw, wcounts), flush=True)
dev.close()
