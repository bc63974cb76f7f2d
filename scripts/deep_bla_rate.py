"""Deep-zoom views with bilinear approximation (MBK_DEEP_BLA) against the plain deep kernel: kernel time of a 4096^2 view,
mrd 30 000, on the three views of scripts/deep_rate.py (spans 1e-8 and 1e-20 at the seahorse-valley centre, 1e-60 at c = i).
The two kernels alternate in one process after a clock ramp; times are HIP events (the stats' kernel_ms), the median of
`reps` runs each.  Also printed: the share of steps the BLA rule executes (mbk_deep_bla_count_host on a seeded sample of
pixels, against count or mrd - 1 of the plain kernel's counts there) and the share of pixels whose counts differ between the
two kernels.   python scripts/deep_bla_rate.py [reps] [sample]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, _lib as L

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sample = int(sys.argv[2]) if len(sys.argv) > 2 else 512
mrd, n = 30000, 4096
lib = L.load()
dev = MandelbrotDevice(0)
plain = dev.pinned_empty((n, n), np.int32)
bla = dev.pinned_empty((n, n), np.int32)
for centre, span in ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60)):
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, n)
    for _ in range(2):   # uploads (orbit, table) and the clock ramp
        dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=plain)
        dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=bla, bla=True)
    kp, kb = [], []
    for _ in range(reps):
        kp.append(dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=plain)[3].kernel_ms)
        st = dev.compute_deep_view(orbit, view, mrd, want_bytes=False, out_counts=bla, bla=True)[3]
        kb.append(st.kernel_ms)
    pick = np.random.RandomState(3).choice(n * n, sample, replace=False)
    cv = L.mbk_deep_view(view.span_r, view.span_i, n, n, 0, 0, n, n)
    steps = 0
    for p in pick:
        cc, mm, ss = C.c_int32(), C.c_double(), C.c_uint64()
        assert lib.mbk_deep_bla_count_host(orbit._h, C.byref(cv), int(p % n), int(p // n), mrd, C.byref(cc), C.byref(mm),
                                           C.byref(ss)) == L.MBK_OK
        assert cc.value == bla.ravel()[p], (int(p), cc.value, int(bla.ravel()[p]))
        steps += ss.value
    pc = plain.ravel()[pick].astype(np.int64)
    full = int(np.where(pc > 0, pc, mrd - 1).sum())
    p_ms, b_ms = float(np.median(kp)), float(np.median(kb))
    print(f"span {span:g} centre ({centre[0][:12]}, {centre[1][:12]}) M {orbit.length}: plain kernel ms median {p_ms:.2f} "
          f"(min {min(kp):.2f}), BLA {b_ms:.2f} (min {min(kb):.2f}), BLA / plain {b_ms / p_ms:.3f}; steps executed / plain "
          f"steps on {sample} pixels {steps / full:.3f}; pixels whose counts differ {100.0 * (plain != bla).mean():.4f} %; "
          f"pixel-steps {st.pixel_iterations:,}", flush=True)
dev.close()
