"""Deep-zoom views (mbk_deep_view_*): kernel time and executed pixel-steps/s of a 4096^2 view, mrd 30 000, at spans 1e-8,
1e-20 (the seahorse-valley centre of tests/test_deep_orbit.py) and 1e-60 (c = i: a boundary point at every depth; the
seahorse centre is given to 33 digits only).  Every pixel runs count (or mrd - 1) steps -- there is no cycle test here -- so
the executed steps are the stats' pixel_iterations.   python scripts/deep_rate.py [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mrd, n = 30000, 4096
dev = MandelbrotDevice(0)
counts = dev.pinned_empty((n, n), np.int32)
for centre, span in ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60)):
    t0 = time.perf_counter()
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    t_orbit = time.perf_counter() - t0
    view = DeepView(span, n)
    dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=counts)   # upload + warm-up
    ks, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, _, _, st = dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=counts)
        walls.append(time.perf_counter() - t0)
        ks.append(st.kernel_ms)
    k = float(np.median(ks))
    print(f"span {span:g} centre ({centre[0][:12]}, {centre[1][:12]}) P {orbit.precision_bits} M {orbit.length}: orbit {t_orbit * 1e3:.1f} ms host; "
          f"kernel ms median {k:.2f} (min {min(ks):.2f}, wall {np.median(walls) * 1e3:.1f}); pixel-steps {st.pixel_iterations:,} "
          f"= {st.pixel_iterations / (k * 1e-3) / 1e12:.3f} T/s; never escaped {st.never_pixels}; distinct counts {len(np.unique(counts))}",
          flush=True)
dev.close()
