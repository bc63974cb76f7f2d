"""The deep-zoom contract of include/mbk.h ("Deep-zoom views") restated for the tests -- a helper module, not a conftest.

* offsets(): the pixel offsets dc of a view / window, fl(fl(k - (W-1)/2) * fl(R / (W-1))), as float64 numpy operations;
* model_counts(): perturbation with rebasing, vectorised over pixels, every operation a separate float64 numpy operation
  (numpy never contracts), on the orbit table mbk_deep_orbit_read returns -- the GPU must equal it bit for bit;
* direct_counts(): the same pixels iterated directly, z = z^2 + c from z = c, in fixed point with Python integers at a
  precision of the caller's choice -- the ground truth the model is compared with (a tolerance, on the CPU).
"""
from __future__ import annotations

from decimal import Decimal
from fractions import Fraction

import numpy as np


def axis_offsets(n: int, span: float, k) -> np.ndarray:
    k = np.asarray(k, dtype=np.float64)
    if n <= 1:
        return np.zeros_like(k)
    s = np.float64(span) / np.float64(n - 1)
    return (k - np.float64((n - 1) / 2)) * s


def offsets(view, window=None):
    """(dcr, dci) of every pixel of the window, row-major (real axis fastest)."""
    col0, row0, ncols, nrows = window if window is not None else (0, 0, view.width, view.height)
    dr = axis_offsets(view.width, view.span_r, np.arange(col0, col0 + ncols))
    di = axis_offsets(view.height, view.span_i, np.arange(row0, row0 + nrows))
    return np.tile(dr, nrows), np.repeat(di, ncols)


def model_counts(zr, zi, dcr, dci, mrd: int, on_step=None):
    """(counts int32, |z|^2 at the escaping step float64) of the pixels with offsets (dcr, dci).  on_step, if given, sees
    the new offsets (dz.r, dz.i) of the live pixels after every step."""
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    M = zr.size - 1
    z2r, z2i = zr + zr, zi + zi
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    n = cr.size
    count = np.zeros(n, np.int32)
    mag = np.zeros(n, np.float64)
    idx = np.arange(n)
    m = np.ones(n, np.int64)
    dr, di = cr.copy(), ci.copy()
    if M == 1:
        dr, di = zr[1] + cr, zi[1] + ci
        m[:] = 0
    for i in range(1, mrd):
        if idx.size == 0:
            break
        ar = z2r[m] + dr
        ai = z2i[m] + di
        ndr = (ar * dr - ai * di) + cr
        ndi = (ar * di + ai * dr) + ci
        m = m + 1
        if on_step is not None:
            on_step(ndr, ndi)
        xr = zr[m] + ndr
        xi = zi[m] + ndi
        mg = xr * xr + xi * xi
        esc = mg >= 4.0
        if esc.any():
            count[idx[esc]] = i
            mag[idx[esc]] = mg[esc]
            keep = ~esc
            idx, cr, ci, ndr, ndi, m, xr, xi, mg = (a[keep] for a in (idx, cr, ci, ndr, ndi, m, xr, xi, mg))
        reb = (mg < ndr * ndr + ndi * ndi) | (m == M)
        dr = np.where(reb, xr, ndr)
        di = np.where(reb, xi, ndi)
        m = np.where(reb, 0, m)
    return count, mag


def smooth_from(count, mag):
    """n + 1 - log2(0.5 ln |z_n|^2) with libm's logs; 0 for count 0."""
    out = np.zeros(count.shape, np.float64)
    e = count > 0
    out[e] = count[e] + 1.0 - np.log2(0.5 * np.log(mag[e]))
    return out


def exact(x) -> Fraction:
    return Fraction(Decimal(x)) if isinstance(x, str) else Fraction(x)


def direct_count(c_r: Fraction, c_i: Fraction, mrd: int, bits: int) -> int:
    """calc_mb_value's count for c, iterated in fixed point with `bits` fraction bits (products floored)."""
    cr = (c_r.numerator << bits) // c_r.denominator
    ci = (c_i.numerator << bits) // c_i.denominator
    zr, zi = cr, ci
    a, b = (zr * zr) >> bits, (zi * zi) >> bits
    four = 4 << bits
    for n in range(1, mrd):
        zi = ((zr * zi) >> (bits - 1)) + ci
        zr = a - b + cr
        a, b = (zr * zr) >> bits, (zi * zi) >> bits
        if a + b >= four:
            return n
    return 0


def direct_counts(center_r: str, center_i: str, dcr, dci, mrd: int, bits: int) -> np.ndarray:
    Cr, Ci = exact(center_r), exact(center_i)
    return np.array([direct_count(Cr + Fraction(float(x)), Ci + Fraction(float(y)), mrd, bits) for x, y in zip(dcr, dci)],
                    np.int32)


def fixed_orbit(center_r: str, center_i: str, P: int, mrd: int):
    """The contract's reference orbit at P fraction bits, restated with Python integers: (Z as Fractions, M, escaped)."""
    def parse(s):
        v = exact(s)
        mag = (abs(v.numerator) << P) // v.denominator
        return -mag if v < 0 else mag

    def mul(a, b):
        p = (abs(a) * abs(b)) >> P
        return -p if (a < 0) != (b < 0) else p

    Cr, Ci = parse(center_r), parse(center_i)
    zr = zi = 0
    out = [(0, 0)]
    k = 0
    while True:
        sr, si, t = mul(zr, zr), mul(zi, zi), mul(zr, zi)
        if k > 0 and sr + si >= (4 << P):
            return out, k, True
        if k == mrd:
            return out, k, False
        zr, zi = sr - si + Cr, t + t + Ci
        k += 1
        out.append((zr, zi))
