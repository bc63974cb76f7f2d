"""Distance estimates for deep views (mbk_deep_view_launch_distance) beside the deep kernel they ride on (mbk_deep_view_launch,
counts + smooth), on the three views of scripts/deep_rate.py: 4096^2, mrd 30 000, spans 1e-8 and 1e-20 (seahorse valley) and
1e-60 (c = i).  Kernel time from HIP events on one stream, median of `reps`, the two kernels alternating after a clock ramp of
~2 s of the deep kernel; the share of pixel-steps that belong to never-escaping pixels, from the counts; and the wall time of a
1024^2 render of the 1e-60 view at s = 1 and s = 2 with sources "smooth" and "distance_rel".
    python scripts/deep_distance_rate.py [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, Palette

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
mrd, n = 30000, 4096
dev = MandelbrotDevice(0)
d_counts = torch.empty(n * n, dtype=torch.int32, device="cuda:0")
d_val = torch.empty(n * n, dtype=torch.float64, device="cuda:0")
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
    deep = lambda: dev.launch_deep_view(orbit, view, mrd, d_counts=d_counts.data_ptr(), d_smooth=d_val.data_ptr(), stream=stream.cuda_stream)
    dist = lambda: dev.launch_deep_view_distance(orbit, view, mrd, d_rel=d_val.data_ptr(), d_counts=d_counts.data_ptr(), stream=stream.cuda_stream)
    deep()
    dist()           # upload + warm-up of both
    stream.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 2.0:          # the clock ramp
        timed(deep)
    a, b = [], []
    for _ in range(reps):
        a.append(timed(deep))
        b.append(timed(dist))
    counts = d_counts.cpu().numpy().astype(np.int64)
    steps = np.where(counts > 0, counts, mrd - 1)
    interior = float(steps[counts == 0].sum()) / float(steps.sum())
    ka, kb = float(np.median(a)), float(np.median(b))
    print(f"span {span:g} P {orbit.precision_bits} M {orbit.length}: deep (counts + smooth) {ka:.2f} ms (min {min(a):.2f}), distance {kb:.2f} ms "
          f"(min {min(b):.2f}), ratio {kb / ka:.3f}; pixel-steps {int(steps.sum()):,} = {steps.sum() / (kb * 1e-3) / 1e12:.3f} T/s with the derivative; "
          f"never-escaping pixels {int((counts == 0).sum())} hold {100 * interior:.2f} % of the pixel-steps", flush=True)

orbit = DeepOrbit("0", "1", mrd, min_span=1e-60)
view = DeepView(1e-60, 1024)
for s in (1, 2):
    for source, pal in (("smooth", Palette.cosine()), ("distance_rel", Palette.deep_distance(view, 8.0))):
        dev.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            img, st = dev.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s)
            walls.append(time.perf_counter() - t0)
        print(f"render 1024^2 of the 1e-60 view, s = {s}, source {source}: wall {np.median(walls) * 1e3:.1f} ms, kernel {st.kernel_ms:.1f} ms, "
              f"{len(np.unique(img.reshape(-1, 4), axis=0))} colours", flush=True)
dev.close()
