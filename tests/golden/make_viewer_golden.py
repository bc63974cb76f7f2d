#!/usr/bin/env python3
"""Generate tests/golden/viewer_palette.npz by EXECUTING THE REFERENCE VIEWER'S OWN SOURCE.

Run once, where the reference tree and matplotlib are at hand (neither a test nor the package needs them):

    python tests/golden/make_viewer_golden.py <reference root>

The reference's Viewer (DistributedMandelbrotViewer/DistributedMandelbrotViewer.py, "Viewer.py") colours a chunk in
``data_to_img_array`` (:110-135): bytes / 256, inverted, through matplotlib's ``jet``, black where the byte is 0.  The
unmodified file is loaded from where it lies (matplotlib on the Agg backend, so that importing pyplot opens no window) and
called on one 4096 x 4096 array that holds every byte value; recorded are the 256 distinct float64 RGBA rows it returns,
by byte value, and their 8-bit form floor(255 x + 0.5) -- the rounding mbk_palette_viewer documents (include/mbk.h).
Nothing from the reference is copied into this repository: only these outputs are stored.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "viewer_palette.npz")


def main(root: str) -> None:
    import matplotlib
    matplotlib.use("Agg")
    path = os.path.join(root, "DistributedMandelbrotViewer", "DistributedMandelbrotViewer.py")
    spec = importlib.util.spec_from_file_location("reference_viewer", path)
    viewer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(viewer)   # guarded by __name__ == "__main__": defines functions only

    n = viewer.CHUNK_WIDTH * viewer.CHUNK_WIDTH
    data = (np.arange(n, dtype=np.int64) * 7 % 256).astype(np.uint8)   # every byte value, 65536 times each, interleaved
    img = viewer.data_to_img_array(data).reshape(n, 4)
    assert img.dtype == np.float64
    rgba = np.empty((256, 4), np.float64)
    for b in range(256):
        rows = img[data == b]
        assert (rows == rows[0]).all()   # the colour is a function of the byte alone
        rgba[b] = rows[0]
    rgba8 = np.floor(255.0 * rgba + 0.5).astype(np.uint8)
    ties = int((255.0 * rgba == np.floor(255.0 * rgba) + 0.5).sum())
    np.savez_compressed(OUT, rgba=rgba, rgba8=rgba8, matplotlib_version=np.array(matplotlib.__version__),
                        numpy_version=np.array(np.__version__))
    print(f"{OUT}: 256 rows, {len(np.unique(rgba8, axis=0))} distinct 8-bit colours, {ties} channel values on a .5 tie, "
          f"matplotlib {matplotlib.__version__}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
