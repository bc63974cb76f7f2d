"""Distance estimates for extended-range deep views: kernel time of deep_wide_distance_kernel (launch_wide_view_distance)
beside deep_wide_kernel (launch_deep_view, counts only) on the same WideDeepView in the same run -- c = i at range 1,
exp2 = -1100, mrd 3000, n x n with n large enough that a launch runs >= 50 ms.  Both are launched on one torch stream between
HIP events; a clock ramp of `ramp` untimed launches of each comes first, then `legs` legs in which the two alternate, `reps`
launches each per leg; the figure of a kernel is the median over all its timed launches, and the spread over the legs'
medians is printed beside it.   python scripts/deep_wide_distance_rate.py [n] [legs] [reps] [ramp]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, WideDeepView

n = int(sys.argv[1]) if len(sys.argv) > 1 else 6144
legs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ramp = int(sys.argv[4]) if len(sys.argv) > 4 else 3
mrd = 3000
dev = MandelbrotDevice(0)
view = WideDeepView(1.0, -1100, n)
orbit = DeepOrbit("0", "1", mrd, min_span_exp2=view.min_span_exp2)
stream = torch.cuda.Stream(device="cuda:0")
counts = torch.zeros(n * n, dtype=torch.int32, device="cuda:0")
dcounts = torch.zeros(n * n, dtype=torch.int32, device="cuda:0")
rel = torch.zeros(n * n, dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()


def wide():
    dev.launch_deep_view(orbit, view, mrd, d_counts=counts.data_ptr(), stream=stream.cuda_stream)


def distance():
    dev.launch_wide_view_distance(orbit, view, mrd, d_rel=rel.data_ptr(), d_counts=dcounts.data_ptr(), stream=stream.cuda_stream)


def timed(launch) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    launch()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1)


for _ in range(ramp):     # the first launch uploads the wide table; the rest bring the clocks up
    timed(wide)
    timed(distance)
ms = {"wide": [], "distance": []}
for _ in range(legs):
    for name, launch in (("wide", wide), ("distance", distance)):
        ms[name].append([timed(launch) for _ in range(reps)])
c = counts.cpu().numpy()
assert np.array_equal(c, dcounts.cpu().numpy())
r = rel.cpu().numpy()
steps = int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
print(f"{torch.cuda.get_device_name(0)}: c = i, range 1, exp2 -1100, {n} x {n}, mrd {mrd}, P {orbit.precision_bits}: {steps:,} counted "
      f"pixel-steps, {int((c == 0).sum())} never escaped, counts equal; rel finite and > 0 on "
      f"{float((np.isfinite(r) & (r > 0))[c > 0].mean()) * 100:.4f} % of escaped pixels")
med = {}
for name, rows in ms.items():
    a = np.array(rows)
    med[name] = float(np.median(a))
    per_leg = np.median(a, axis=1)
    print(f"  {name}: kernel ms median {med[name]:.2f} over {a.size} launches (min {a.min():.2f}, max {a.max():.2f}; legs' medians "
          f"{per_leg.min():.2f} .. {per_leg.max():.2f}) = {steps / (med[name] * 1e-3) / 1e12:.3f} T counted steps/s")
print(f"  distance / wide: {med['distance'] / med['wide']:.3f}", flush=True)
dev.close()
