"""Distance estimates for deep views with bilinear approximation (mbk_deep_view_compute_distance_bla) against the plain deep
distance kernel (mbk_deep_view_compute_distance): kernel time of a 4096^2 view, mrd 30 000, on the three views of
scripts/deep_rate.py (spans 1e-8 and 1e-20 at the seahorse-valley centre, 1e-60 at c = i).  deep_distance_kernel and
deep_distance_bla_kernel alternate in one process after two warm-up rounds (uploads of orbit and table, the clock ramp); times
are HIP events (the stats' kernel_ms), the median of `reps` runs each.  Also printed: the share of steps the rule executes
(mbk_deep_distance_bla_host on a seeded sample of pixels, against count or mrd - 1 there), the share of pixels whose counts
differ between the two kernels, and the largest relative difference of rel between them on the sample.
    timeout -k 10 300 python scripts/deep_distance_bla_rate.py [reps] [sample]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, deep_distance_bla_host

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sample = int(sys.argv[2]) if len(sys.argv) > 2 else 256
mrd, n = 30000, 4096
dev = MandelbrotDevice(0)
for centre, span in ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60)):
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, n)
    for _ in range(2):   # uploads (orbit, table) and the clock ramp
        dev.compute_deep_view_distance(orbit, view, mrd)
        dev.compute_deep_view_distance_bla(orbit, view, mrd)
    kp, kb = [], []
    for _ in range(reps):
        prel, pc, st = dev.compute_deep_view_distance(orbit, view, mrd)
        kp.append(st.kernel_ms)
        brel, bc, st = dev.compute_deep_view_distance_bla(orbit, view, mrd)
        kb.append(st.kernel_ms)
    pick = np.random.RandomState(3).choice(n * n, sample, replace=False)
    host = deep_distance_bla_host(orbit, view, pick, mrd)
    assert np.array_equal(host["n"], bc.ravel()[pick])
    c = pc.ravel()[pick].astype(np.int64)
    full = int(np.where(c > 0, c, mrd - 1).sum())
    both = (c > 0) & (bc.ravel()[pick] == c)
    with np.errstate(all="ignore"):
        drel = np.abs(brel.ravel()[pick][both] - prel.ravel()[pick][both]) / prel.ravel()[pick][both]
    p_ms, b_ms = float(np.median(kp)), float(np.median(kb))
    print(f"span {span:g} centre ({centre[0][:12]}, {centre[1][:12]}) M {orbit.length}: deep_distance_kernel ms median {p_ms:.2f} "
          f"(min {min(kp):.2f}), deep_distance_bla_kernel {b_ms:.2f} (min {min(kb):.2f}), BLA / plain {b_ms / p_ms:.3f}; steps executed / "
          f"iterations on {sample} pixels {int(host['steps'].sum()) / full:.3f}; pixels whose counts differ "
          f"{100.0 * (pc != bc).mean():.4f} %; largest |rel_bla - rel| / rel on the sample {float(drel.max()) if drel.size else 0.0:.2e} "
          f"(median {float(np.median(drel)) if drel.size else 0.0:.2e}); pixel-steps {st.pixel_iterations:,}", flush=True)
dev.close()
