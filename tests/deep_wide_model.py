"""The extended-range deep contract of include/mbk.h ("Extended-range deep views") restated for the tests -- a helper
module, not a conftest.

* wide_table(): the wide orbit table (X_r, X_i, xe), Z_m = X 2^xe, from Python integers (deep_model.fixed_orbit);
* offsets(): the mantissa offsets dcm of a wide view / window -- the plain contract's formula applied to range_*;
* model_counts(): the step (a) .. (g) of the header, vectorised over pixels, every operation a separate float64 numpy
  operation on binary64 mantissas and int64 exponents -- the host twin and the GPU must equal it bit for bit;
* direct_counts(): the ground truth, deep_model.direct_count on the exact offsets dcm 2^exp2.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import deep_model as D

EZ = -(1 << 24)   # the exponent of a zero


def wide_table(center_r: str, center_i: str, P: int, mrd: int):
    """(X_r float64, X_i float64, xe int32) of Z_0 .. Z_M: xe is the bit length of the larger |component| minus P, each
    component the fixed-point integer over 2^(P + xe), rounded to nearest-even binary64 (int / int is correctly rounded)."""
    Z, M, _ = D.fixed_orbit(center_r, center_i, P, mrd)
    xr = np.zeros(M + 1, np.float64)
    xi = np.zeros(M + 1, np.float64)
    xe = np.full(M + 1, EZ, np.int32)
    for k, (a, b) in enumerate(Z):
        H = max(abs(a).bit_length(), abs(b).bit_length())
        if H:
            xr[k], xi[k], xe[k] = a / (1 << H), b / (1 << H), H - P
    return xr, xi, xe


def offsets(view, window=None):
    """(dcm_r, dcm_i) of every pixel of the window, row-major: the offsets are dcm 2^exp2."""
    col0, row0, ncols, nrows = window if window is not None else (0, 0, view.width, view.height)
    dr = D.axis_offsets(view.width, view.range_r, np.arange(col0, col0 + ncols))
    di = D.axis_offsets(view.height, view.range_i, np.arange(row0, row0 + nrows))
    return np.tile(dr, nrows), np.repeat(di, ncols)


def sh(x, k):
    return np.ldexp(x, np.maximum(k, -1200).astype(np.int32))


def norm(vr, vi, e):
    mx = np.maximum(np.abs(vr), np.abs(vi))
    _, s = np.frexp(mx)
    s = s.astype(np.int64)
    zero = mx == 0.0
    wr = np.where(zero, 0.0, np.ldexp(vr, (-s).astype(np.int32)))
    wi = np.where(zero, 0.0, np.ldexp(vi, (-s).astype(np.int32)))
    return wr, wi, np.where(zero, EZ, e + s)


def _z(Xr, Xi, xe, wr, wi, q):
    """step (e): t, zv, mg"""
    t = np.maximum(xe, q)
    zr = sh(Xr, xe - t) + sh(wr, q - t)
    zi = sh(Xi, xe - t) + sh(wi, q - t)
    return t, zr, zi, zr * zr + zi * zi


def model_counts(xr, xi, xe, dcr, dci, exp2: int, mrd: int):
    """(counts int32, mag float64 at the escaping step) of the pixels with mantissa offsets (dcr, dci) 2^exp2."""
    xr = np.asarray(xr, np.float64)
    xi = np.asarray(xi, np.float64)
    xe = np.asarray(xe, np.int64)
    M = xr.size - 1
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    n = cr.size
    count = np.zeros(n, np.int32)
    mag = np.zeros(n, np.float64)
    idx = np.arange(n)
    m = np.ones(n, np.int64)
    wr, wi, q = norm(cr, ci, np.full(n, exp2, np.int64))
    if M == 1:
        t, zr, zi, _ = _z(xr[m], xi[m], xe[m], wr, wi, q)
        wr, wi, q = norm(zr, zi, t)
        m[:] = 0
    for i in range(1, mrd):
        if idx.size == 0:
            break
        # a
        x1 = xe[m] + 1
        g = np.maximum(x1, q)
        Ar = sh(xr[m], x1 - g) + sh(wr, q - g)
        Ai = sh(xi[m], x1 - g) + sh(wi, q - g)
        # b
        pr = Ar * wr - Ai * wi
        pi = Ar * wi + Ai * wr
        pe = g + q
        # c
        h = np.maximum(pe, exp2)
        Nr = sh(pr, pe - h) + sh(cr, exp2 - h)
        Ni = sh(pi, pe - h) + sh(ci, exp2 - h)
        # d
        wr, wi, q = norm(Nr, Ni, h)
        m = m + 1
        # e
        t, zr, zi, mg = _z(xr[m], xi[m], xe[m], wr, wi, q)
        mgs = np.ldexp(mg, (2 * np.maximum(t, -600)).astype(np.int32))
        # f
        esc = mgs >= 4.0
        if esc.any():
            count[idx[esc]] = i
            mag[idx[esc]] = mgs[esc]
            keep = ~esc
            idx, cr, ci, wr, wi, q, m, t, zr, zi, mg = (a[keep] for a in (idx, cr, ci, wr, wi, q, m, t, zr, zi, mg))
        # g
        dm = wr * wr + wi * wi
        reb = (mg < np.ldexp(dm, (2 * np.maximum(q - t, -600)).astype(np.int32))) | (m == M)
        if reb.any():
            nr, ni, nq = norm(zr, zi, t)
            wr = np.where(reb, nr, wr)
            wi = np.where(reb, ni, wi)
            q = np.where(reb, nq, q)
            m = np.where(reb, 0, m)
    return count, mag


def direct_counts(center_r: str, center_i: str, dcr, dci, exp2: int, mrd: int, bits: int) -> np.ndarray:
    """The truth: z = z^2 + c from z = c at `bits` fraction bits, c = C + dcm 2^exp2 as exact Fractions."""
    Cr, Ci = D.exact(center_r), D.exact(center_i)
    s = Fraction(1, 1 << -exp2) if exp2 < 0 else Fraction(1 << exp2)
    return np.array([D.direct_count(Cr + Fraction(float(x)) * s, Ci + Fraction(float(y)) * s, mrd, bits)
                     for x, y in zip(dcr, dci)], np.int32)


def as_wide(span_r: float, span_i: float):
    """(range_r, range_i, exp2) naming the plain spans: the larger range in [2, 4), or exp2 = 0."""
    _, e = np.frexp(max(span_r, span_i))
    exp2 = min(int(e) - 2, 0)
    return float(np.ldexp(span_r, -exp2)), float(np.ldexp(span_i, -exp2)), exp2
