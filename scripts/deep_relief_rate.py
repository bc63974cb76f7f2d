"""Relief shading for deep views (mbk_deep_view_launch_normal, mbk_deep_view_relief_render_compute) against the deep distance
calls it shares its loops with, on the three views of scripts/deep_rate.py (spans 1e-8 and 1e-20 at the seahorse-valley centre,
1e-60 at c = i; mrd 30 000).

Kernels (4096^2): deep_relief_kernel against deep_distance_kernel and deep_relief_bla_kernel against deep_distance_bla_kernel,
launch forms into device buffers on one torch stream.  A leg is r back-to-back launches between two events, r chosen so that a
leg lasts at least 60 ms; the legs of a view alternate, `reps` times, after two warm-up rounds (uploads of orbit and table, the
clock ramp).  Printed per leg: the median time of one launch, and the spread (min .. max) over the reps.  The relief kernel is
timed with the outputs a render band asks for (counts, nu, normals) and with rel as well.

Renders (1024^2 output, supersample 2): render_deep_view_relief against render_deep_view(source="smooth") plus
compute_deep_view_distance[_bla] of the same view -- what a caller pays today for the samples a relief needs -- wall time around
r synchronous calls, the same alternation.
    timeout -k 10 420 python scripts/deep_relief_rate.py [reps]"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, Palette

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
VIEWS = ((SEAHORSE, 1e-8), (SEAHORSE, 1e-20), (("0", "1"), 1e-60))
LEG_MS = 60.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
mrd, n = 30000, 4096
dev = MandelbrotDevice(0)
stream = torch.cuda.Stream(device="cuda:0")
px = n * n
d_counts = torch.empty(px, dtype=torch.int32, device="cuda:0")
d_normals = torch.empty(2 * px, dtype=torch.float64, device="cuda:0")
d_nu = torch.empty(px, dtype=torch.float64, device="cuda:0")
d_rel = torch.empty(px, dtype=torch.float64, device="cuda:0")
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


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


print(f"kernels, {n}^2, mrd {mrd}, median of {reps} legs of >= {LEG_MS:.0f} ms (min .. max)", flush=True)
for centre, span in VIEWS:
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, n)
    pc, pn, pu, pr, s = d_counts.data_ptr(), d_normals.data_ptr(), d_nu.data_ptr(), d_rel.data_ptr(), stream.cuda_stream
    legs = {
        "distance": lambda: dev.launch_deep_view_distance(orbit, view, mrd, d_rel=pr, d_counts=pc, stream=s),
        "relief": lambda: dev.launch_deep_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, stream=s),
        "relief+rel": lambda: dev.launch_deep_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, d_rel=pr, stream=s),
        "distance_bla": lambda: dev.launch_deep_view_distance_bla(orbit, view, mrd, d_rel=pr, d_counts=pc, stream=s),
        "relief_bla": lambda: dev.launch_deep_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, stream=s, bla=True),
        "relief_bla+rel": lambda: dev.launch_deep_view_normals(orbit, view, mrd, d_normals=pn, d_counts=pc, d_smooth=pu, d_rel=pr, stream=s,
                                                               bla=True),
    }
    res = alternate(legs, leg_events)
    print(f"span {span:g} M {orbit.length}: {show(res)}; relief / distance {res['relief'][0] / res['distance'][0]:.4f}, "
          f"relief_bla / distance_bla {res['relief_bla'][0] / res['distance_bla'][0]:.4f}", flush=True)

w = 1024
pal = Palette(np.random.RandomState(5).randint(0, 256, (256, 4)).astype(np.uint8), inside=(0, 0, 0, 255))
out = np.empty((w, w, 4), np.uint8)
print(f"renders, {w}^2 output, supersample 2, mrd {mrd}, wall time, median of {reps} legs of >= {LEG_MS:.0f} ms (min .. max)", flush=True)
for centre, span in VIEWS[1:]:
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, w)
    for bla in (False, True):
        distance = dev.compute_deep_view_distance_bla if bla else dev.compute_deep_view_distance
        legs = {
            "relief render": lambda: dev.render_deep_view_relief(orbit, view, mrd, palette=pal, supersample=2, bla=bla, out=out),
            "smooth render": lambda: dev.render_deep_view(orbit, view, mrd, palette=pal, source="smooth", supersample=2, bla=bla, out=out),
            "distance values": lambda: distance(orbit, view, mrd),
        }
        res = alternate(legs, leg_wall)
        both = res["smooth render"][0] + res["distance values"][0]
        print(f"span {span:g} bla {bla}: {show(res)}; relief / (smooth + distance) {res['relief render'][0] / both:.3f}", flush=True)
dev.close()
