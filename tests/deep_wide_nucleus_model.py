"""The contract of include/mbk.h, "Locating minibrots in extended-range deep views", in numpy, and its truth -- a helper module,
not a conftest.  Written from the header's text, not from the C code; built on the derivative step, the z step and the rebase of
deep_wide_distance_model.

    nmag    nmag(mg, t) = (bm, be): s = frexp exponent of mg, bm = ldexp(mg, -s), be = 2t + s; mg == 0: (0, -2^30)
            (bm', be') < (bm, be) iff be' < be, or be' == be and bm' < bm
    start   best = nmag of z_0's (mg, t), arg = 0, z_b = (zv, t) of z_0 = c, (D_b, e_b) = (0.5, 0, 1)
    step i  dstep, steps (a) .. (e); mag >= 4: n = i, the pixel ends (never a candidate);
            nmag(mg, t) < best (strict): best, arg = i, z_b = (zv, t), (D_b, e_b) = (D, e); then (g)
    period  arg + 1
    delta   den = fl(fl(D_b.r^2) + fl(D_b.i^2)), N = (fl(fl(z_b.r D_b.r) + fl(z_b.i D_b.i)), fl(fl(z_b.i D_b.r) - fl(z_b.r D_b.i)))
            delta = ldexp(-fl(fl(N / den) / f), t_b - e_b - k - exp2), range_r = f 2^k; a non-finite component: both +inf

numpy rounds every operation on its own, so every value is the contract's bit for bit.  hp_argmin() runs z' = z^2 + c in mpmath
from the exact c = C + dcm 2^exp2 and returns the two smallest |z_n|^2.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

import deep_model as D
import deep_wide_distance_model as WD
import deep_wide_model as W

NMAG_ZERO_EXP = -(1 << 30)


def nmag(mg, t):
    """(bm float64, be int64) of arrays mg, t"""
    mg = np.asarray(mg, np.float64)
    _, s = np.frexp(mg)
    s = s.astype(np.int64)
    zero = mg == 0.0
    bm = np.where(zero, 0.0, np.ldexp(mg, (-s).astype(np.int32)))
    be = np.where(zero, NMAG_ZERO_EXP, 2 * np.asarray(t, np.int64) + s)
    return bm, be


def less(bm1, be1, bm, be):
    return (be1 < be) | ((be1 == be) & (bm1 < bm))


def delta(zr, zi, t, Dr, Di, e, range_r, exp2):
    """The output expression on arrays: float64[N, 2]."""
    f, k = math.frexp(float(range_r))
    with np.errstate(all="ignore"):
        r2 = Dr * Dr
        i2 = Di * Di
        den = r2 + i2
        a0 = zr * Dr
        a1 = zi * Di
        b0 = zi * Dr
        b1 = zr * Di
        nr = a0 + a1
        ni = b0 - b1
        gr = (nr / den) / np.float64(f)
        gi = (ni / den) / np.float64(f)
        sh = np.asarray(t, np.int64) - np.asarray(e, np.int64) - k - int(exp2)
        sh = np.clip(sh, -(1 << 30), 1 << 30).astype(np.int32)        # (beyond +-2^12 every shift gives the same 0 or inf)
        xr = np.ldexp(-gr, sh)
        xi = np.ldexp(-gi, sh)
    bad = ~(np.isfinite(xr) & np.isfinite(xi))
    return np.stack([np.where(bad, np.inf, xr), np.where(bad, np.inf, xi)], axis=1)


def states(xr, xi, xe, dcr, dci, exp2: int, mrd: int):
    """Wide orbit table and flat mantissa offsets -> dict of flat arrays: n, period (int32), best_m, best_e (int64), z [N, 2],
    t (int64), D [N, 2], e (int64)."""
    T = (np.asarray(xr, np.float64), np.asarray(xi, np.float64), np.asarray(xe, np.int64))
    M = T[0].size - 1
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    with np.errstate(all="ignore"):
        idx = np.arange(N)
        m = np.ones(N, np.int64)
        wr, wi, q = W.norm(cr, ci, np.full(N, exp2, np.int64))
        t, zr, zi, mg = W._z(T[0][m], T[1][m], T[2][m], wr, wi, q)     # z_0 = c
        best_m, best_e = nmag(mg, t)
        arg = np.zeros(N, np.int32)
        bz = np.stack([zr, zi], axis=1)
        bt = np.array(t, np.int64)
        if M == 1:
            wr, wi, q = W.norm(zr, zi, t)
            m[:] = 0
        Dr, Di, e = W.norm(np.ones(N), np.zeros(N), np.zeros(N, np.int64))
        bD = np.stack([Dr, Di], axis=1)
        be = np.array(e, np.int64)
        c_r, c_i = cr, ci
        for i in range(1, int(mrd)):
            if idx.size == 0:
                break
            Dr, Di, e = WD.dstep(zr, zi, t, Dr, Di, e)
            wr, wi, q, m, zr, zi, t, mg, mag = WD._zstep(T, wr, wi, q, m, c_r, c_i, exp2)
            esc = mag >= 4.0
            if esc.any():
                n[idx[esc]] = i
                keep = ~esc
                idx, c_r, c_i, Dr, Di, e, wr, wi, q, m, zr, zi, t, mg = (a[keep] for a in (idx, c_r, c_i, Dr, Di, e, wr, wi, q, m,
                                                                                          zr, zi, t, mg))
            cm, ce = nmag(mg, t)
            win = less(cm, ce, best_m[idx], best_e[idx])
            w = idx[win]
            best_m[w], best_e[w], arg[w] = cm[win], ce[win], i
            bz[w, 0], bz[w, 1], bt[w] = zr[win], zi[win], t[win]
            bD[w, 0], bD[w, 1], be[w] = Dr[win], Di[win], e[win]
            wr, wi, q, m = WD._rebase(M, wr, wi, q, m, zr, zi, t, mg)
    return {"n": n, "period": (arg + 1).astype(np.int32), "best_m": best_m, "best_e": best_e.astype(np.int64), "z": bz, "t": bt,
            "D": bD, "e": be}


def model(orbit, view, mrd, window=None):
    """The states of a WideDeepView on a DeepOrbit with delta [N, 2] added, arrays flat in the window's image order."""
    dcr, dci = W.offsets(view, window)
    st = states(*orbit.wide_table(), dcr, dci, view.exp2, mrd)
    st["delta"] = delta(st["z"][:, 0], st["z"][:, 1], st["t"], st["D"][:, 0], st["D"][:, 1], st["e"], view.range_r, view.exp2)
    return st


def hp_argmin(centre, dcm_r, dcm_i, exp2, mrd, bits):
    """z_0 = c, z' = z^2 + c at `bits` bits from the exact c = C + dcm 2^exp2, steps 1 .. mrd - 1 up to the escape: (the step of
    the smallest |z_n|^2 among the steps that did not escape -- the first one if equal --, the smallest and the second smallest
    |z_n|^2 as mpf)."""
    s = Fraction(1, 1 << -exp2) if exp2 < 0 else Fraction(1 << exp2)
    Cr, Ci = D.exact(centre[0]) + Fraction(float(dcm_r)) * s, D.exact(centre[1]) + Fraction(float(dcm_i)) * s
    with mpmath.workprec(bits):
        c = mpmath.mpc(mpmath.mpf(Cr.numerator) / Cr.denominator, mpmath.mpf(Ci.numerator) / Ci.denominator)
        z = c
        first = z.real * z.real + z.imag * z.imag
        arg, second = 0, mpmath.inf
        for i in range(1, int(mrd)):
            z = z * z + c
            mg = z.real * z.real + z.imag * z.imag
            if mg >= 4:
                break
            if mg < first:
                arg, first, second = i, mg, first
            elif mg < second:
                second = mg
        return arg, first, second
