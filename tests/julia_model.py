"""The contract of a Julia view (include/mbk.h, "Julia views") in numpy -- a helper module, not a conftest.

    z_0 = the pixel's coordinate (never tested);  z_(k+1) = z_k^2 + c in binary64, every operation rounded on its own:
        zr' = fl(fl(fl(zr zr) - fl(zi zi)) + c_r),   zi' = fl(fl(fl(2 zr) zi) + c_i)          (the LITERAL form)
    mag_k = fl(fl(zr^2) + fl(zi^2));  n = the first k in 1 .. mrd - 1 with mag_k >= 4 (false for NaN), else 0.

numpy rounds every array operation on its own, so the lines below ARE the contract.  `fma=True` evaluates the kernels'
rewrite zi' = fma(2, fl(zr zi), c_i) instead: 2 p is exact for every binary64 p that does not overflow (a subnormal doubles
exactly), so fl(fl(2 p) + c_i) is the fused result.  The two differ only where zr zi is a non-zero subnormal; the library must
never let that show (it takes the literal loop whenever |c_i| < 2^-900), and tests/test_julia.py keeps cases where it would.
"""
from __future__ import annotations

import numpy as np


def julia_counts(z0r, z0i, c_r, c_i, mrd, fma=False):
    """(n int32, mag float64) per element of the broadcast (z0r, z0i): mag is mag_n of an escaped element, the mag of the
    last step run of one that never escaped, 0 where no step ran (mrd <= 1)."""
    zr, zi = np.broadcast_arrays(np.asarray(z0r, np.float64), np.asarray(z0i, np.float64))
    shape = zr.shape
    zr, zi = zr.reshape(-1).copy(), zi.reshape(-1).copy()
    cr = np.float64(c_r)
    ci = np.float64(c_i)
    n = np.zeros(zr.shape, np.int32)
    mag = np.zeros(zr.shape, np.float64)
    live = np.arange(zr.size)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for k in range(1, int(mrd)):
            if live.size == 0:
                break
            a = zr * zr
            b = zi * zi
            t = a - b
            if fma:
                p = zr * zi
                zi = (np.float64(2.0) * p) + ci
            else:
                w = np.float64(2.0) * zr
                u = w * zi
                zi = u + ci
            zr = t + cr
            m = (zr * zr) + (zi * zi)
            mag[live] = m
            esc = m >= 4.0
            n[live[esc]] = k
            keep = ~esc
            live, zr, zi = live[keep], zr[keep], zi[keep]
    return n.reshape(shape), mag.reshape(shape)


def axes(view, window=None):
    """(re, im) coordinate vectors of a view (start_r, start_i, range_r, range_i, width, height) or a window of it
    (col0, row0, ncols, nrows): np.linspace, as every view."""
    sr, si, rr, ri, w, h = view
    re = np.linspace(sr, sr + rr, w)
    im = np.linspace(si, si + ri, h)
    if window is not None:
        c0, r0, nc, nr = window
        re, im = re[c0:c0 + nc], im[r0:r0 + nr]
    return re, im


def julia_view(view, c, mrd, window=None, fma=False):
    """(n int32[nrows, ncols], mag float64[nrows, ncols]) of the Julia view of c; row 0 is the lowest imaginary part."""
    re, im = axes(view, window)
    return julia_counts(re[None, :], im[:, None], c[0], c[1], mrd, fma=fma)


def quantise(counts, mrd):
    """ceil(count 256 / mrd) mod 256, the quantiser of every view, in integers."""
    c = np.asarray(counts, np.int64)
    return (((c * 256 + mrd - 1) // mrd) % 256).astype(np.uint8)
