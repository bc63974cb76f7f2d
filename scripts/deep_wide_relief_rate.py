"""Relief shading for extended-range deep views (mbk_deep_xview_launch_normal, mbk_deep_xview_relief_render_compute) against
the wide distance calls it shares its loops with, on three views: c = i at range 1, exp2 -1100 (mrd 3000), the Misiurewicz
point of tests/test_deep_wide.py at exp2 -3000 (mrd 9000), and the short orbit of the centre 1e-400 at span 4 (mrd 300), where a
pixel runs so few steps that the per-pixel epilogue shows.

Kernels (n x n, default 4096): deep_wide_relief_kernel against deep_wide_distance_kernel and deep_wide_relief_xbla_kernel
against deep_wide_distance_bla_kernel, launch forms into device buffers on one torch stream.  A leg is r back-to-back launches
between two events, r chosen so that a leg lasts at least 60 ms; the legs of a view alternate, `reps` times, after two warm-up
rounds (uploads of orbit and table, the clock ramp).  Printed per leg: the median time of one launch, and the spread
(min .. max) over the reps.  The relief kernel is timed with the outputs a render band asks for (counts, nu, normals) and with
rel as well.

Renders (1024^2 output, supersample 2), the first two views: render_wide_view_relief against
render_deep_view(source="smooth") plus compute_wide_view_distance[_xbla] of the same view -- what a caller pays today for the
samples a relief needs -- wall time around r synchronous calls, the same alternation.
    timeout -k 10 540 python scripts/deep_wide_relief_rate.py [reps] [n]"""
import math
import os
import sys
import time
from decimal import Decimal, getcontext

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, Palette, WideDeepView


def misiurewicz() -> str:
    """The real root of c^3 + 2c^2 + 2c + 2 to 1300 digits, by Newton (tests/test_deep_wide.py's MIS)."""
    getcontext().prec = 1320
    c = Decimal("-1.5436890126920763615708559718")
    for _ in range(12):
        c = c - (((c + 2) * c + 2) * c + 2) / ((3 * c + 4) * c + 2)
    return str(c.quantize(Decimal(10) ** -1300))


# (name, centre, range, exp2, mrd, precision_bits or None)
VIEWS = (("c = i, 2^-1100", ("0", "1"), 1.0, -1100, 3000, None), ("Misiurewicz, 2^-3000", (misiurewicz(), "0"), 1.0, -3000, 9000, None),
         ("1e-400, span 4", ("1e-400", "0"), 4.0, 0, 300, 1408))
LEG_MS = 60.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
dev = MandelbrotDevice(0)
stream = torch.cuda.Stream(device="cuda:0")
px = n * n
d_counts = torch.empty(px, dtype=torch.int32, device="cuda:0")
d_normals = torch.empty(2 * px, dtype=torch.float64, device="cuda:0")
d_nu = torch.empty(px, dtype=torch.float64, device="cuda:0")
d_rel = torch.empty(px, dtype=torch.float64, device="cuda:0")
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def make_orbit(centre, view, mrd, bits):
    return DeepOrbit(*centre, mrd, precision_bits=bits) if bits else DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)


def leg_events(fn, r):
    """ms per call of r back-to-back launches"""
    t0.record(stream)
    for _ in range(r):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / r


def leg_wall(fn, r):
    """ms per call of r synchronous calls"""
    start = time.perf_counter()
    for _ in range(r):
        fn()
    return 1e3 * (time.perf_counter() - start) / r


def alternate(legs, timer):
    """legs: name -> callable.  Two warm-up rounds, r per leg from the second, then `reps` alternating rounds."""
    for fn in legs.values():
        timer(fn, 1)
    r = {k: max(1, math.ceil(LEG_MS / timer(fn, 1))) for k, fn in legs.items()}
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timer(fn, r[k]))
    return {k: (float(np.median(v)), min(v), max(v), r[k]) for k, v in times.items()}


def show(res):
    return "; ".join(f"{k} {m:.3f} ms ({lo:.3f} .. {hi:.3f}, r {r})" for k, (m, lo, hi, r) in res.items())


print(f"{torch.cuda.get_device_name(0)}: kernels, {n}^2, median of {reps} legs of >= {LEG_MS:.0f} ms (min .. max)", flush=True)
for name, centre, rng, exp2, mrd, bits in VIEWS:
    view = WideDeepView(rng, exp2, n)
    orbit = make_orbit(centre, view, mrd, bits)
    pc, pn, pu, pr, s = d_counts.data_ptr(), d_normals.data_ptr(), d_nu.data_ptr(), d_rel.data_ptr(), stream.cuda_stream
    legs = {
        "distance": lambda: dev.launch_wide_view_distance(orbit, view, mrd, d_rel=pr, d_counts=pc, stream=s),
        "relief": lambda: dev.launch_wide_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, stream=s),
        "relief+rel": lambda: dev.launch_wide_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, d_rel=pr, stream=s),
        "distance_xbla": lambda: dev.launch_wide_view_distance_xbla(orbit, view, mrd, d_rel=pr, d_counts=pc, stream=s),
        "relief_xbla": lambda: dev.launch_wide_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, stream=s, xbla=True),
        "relief_xbla+rel": lambda: dev.launch_wide_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, d_rel=pr, stream=s,
                                                                xbla=True),
    }
    res = alternate(legs, leg_events)
    never = int((d_counts == 0).sum().item())
    print(f"{name}, mrd {mrd}, M {orbit.length}, {never} of {px} never escape: {show(res)}; relief / distance "
          f"{res['relief'][0] / res['distance'][0]:.4f}, relief_xbla / distance_xbla {res['relief_xbla'][0] / res['distance_xbla'][0]:.4f}",
          flush=True)

w = 1024
pal = Palette(np.random.RandomState(5).randint(0, 256, (256, 4)).astype(np.uint8), inside=(0, 0, 0, 255))
out = np.empty((w, w, 4), np.uint8)
print(f"renders, {w}^2 output, supersample 2, wall time, median of {reps} legs of >= {LEG_MS:.0f} ms (min .. max)", flush=True)
for name, centre, rng, exp2, mrd, bits in VIEWS[:2]:
    view = WideDeepView(rng, exp2, w)
    orbit = make_orbit(centre, view, mrd, bits)
    for xbla in (False, True):
        distance = dev.compute_wide_view_distance_xbla if xbla else dev.compute_wide_view_distance
        legs = {
            "relief render": lambda: dev.render_wide_view_relief(orbit, view, mrd, palette=pal, supersample=2, xbla=xbla, out=out),
            "smooth render": lambda: dev.render_deep_view(orbit, view, mrd, palette=pal, source="smooth", supersample=2, xbla=xbla, out=out),
            "distance values": lambda: distance(orbit, view, mrd),
        }
        res = alternate(legs, leg_wall)
        both = res["smooth render"][0] + res["distance values"][0]
        print(f"{name} xbla {xbla}: {show(res)}; relief / (smooth + distance) {res['relief render'][0] / both:.3f}", flush=True)
dev.close()
