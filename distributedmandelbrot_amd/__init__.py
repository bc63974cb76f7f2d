"""MI355X-native Mandelbrot tile worker: a drop-in for the compute path of
ofsouzap/DistributedMandelbrot's worker (DistributedMandelbrotWorkerCUDA.py).

Layout
------
csrc/            hand-written HIP kernels for gfx950 + the C ABI (include/mbk.h) -> libmbk_hip.so
build.py         hipcc driver (in-tree build)
_lib.py          ctypes binding of the C ABI (fails loudly when the library or a GPU is missing)
device.py        MandelbrotDevice: one GPU context; views, DataChunk tiles, async launches
worker.py        the reference worker's interface (process_workload / do_workload_single / main)
                 speaking the unchanged Distributer TCP protocol, plus a per-GPU work-queue farm
image.py         Palette (for MandelbrotDevice.render_view / render_deep_view) and a standard-library PNG writer
viewer.py        the reference Viewer's job: fetch chunk streams from a store or a DataServer and render them, one chunk
                 or a downsampled mosaic of a level, on the GPU (render_level; python -m distributedmandelbrot_amd.viewer)
sharding.py      row-band work items and the per-GPU queue used to shard one view over N GPUs

There is no CPU fallback anywhere in this package.
"""
from .device import DeepOrbit, DeepView, DensityStats, DensityTarget, MandelbrotDevice, MbkError, TileStats, View, WideDeepView, device_count  # noqa: F401
from .device import deep_distance_bla_host, deep_distance_bla_skip_host, deep_normal_host  # noqa: F401
from .device import Nucleus, NucleusError, deep_nucleus_host, locate_nucleus, pick_nucleus_seed, refine_nucleus  # noqa: F401
from .device import locate_wide_nucleus, pick_wide_nucleus_seed, wide_normal_host, wide_nucleus_host, wide_nucleus_precision_bits  # noqa: F401
from .image import Palette, write_png  # noqa: F401

__all__ = ["DeepOrbit", "DeepView", "DensityStats", "DensityTarget", "MandelbrotDevice", "MbkError", "Nucleus", "NucleusError", "Palette",
           "TileStats", "View", "WideDeepView", "deep_distance_bla_host", "deep_distance_bla_skip_host", "deep_normal_host",
           "deep_nucleus_host", "device_count", "locate_nucleus", "locate_wide_nucleus", "pick_nucleus_seed", "pick_wide_nucleus_seed", "refine_nucleus",
           "wide_normal_host", "wide_nucleus_host", "wide_nucleus_precision_bits", "write_png"]
