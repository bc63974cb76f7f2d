"""The contract of include/mbk.h, "Locating minibrots in deep views", in numpy, and its truth -- a helper module, not a
conftest.  Written from the header's text, not from the C code.

    start   best = fl(fl(z_0.r^2) + fl(z_0.i^2)), arg = 0, (z_b, D_b, e_b) = (z_0, (1, 0), 0)          z_0 = c = fl(Z_1 + dc)
    step i  the derivative step and the z step of deep_distance_model; mag >= 4: n = i, the pixel ends (never a candidate);
            mag < best (strict): best = mag, arg = i, z_b = z_i, (D_b, e_b) = (D, e); then the rebase rule
    period  arg + 1
    delta   den = fl(fl(D_b.r^2) + fl(D_b.i^2)), N = (fl(fl(z_b.r D_b.r) + fl(z_b.i D_b.i)), fl(fl(z_b.i D_b.r) - fl(z_b.r D_b.i)))
            delta = ldexp(-fl(fl(N / den) / f), -(e_b + k)), range_r = f 2^k; a non-finite component: both +inf

numpy rounds every operation on its own, so every value is the contract's bit for bit.  hp_argmin() runs z' = z^2 + c in mpmath
from the exact c = C + dc and returns the two smallest |z_n|; hp_newton() is Newton's method on z_p(c) = 0 in mpmath.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

import deep_distance_model as DD
import deep_model as D

TRUTH_BITS = 1400


def delta(zr, zi, Dr, Di, e, range_r):
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
        sh = (-(np.asarray(e, np.int64) + k)).astype(np.int32)
        xr = np.ldexp(-gr, sh)
        xi = np.ldexp(-gi, sh)
    bad = ~(np.isfinite(xr) & np.isfinite(xi))
    return np.stack([np.where(bad, np.inf, xr), np.where(bad, np.inf, xi)], axis=1)


def states(zr, zi, dcr, dci, mrd):
    """Orbit table (zr, zi) and flat offsets -> dict of flat arrays: n, period (int32), best, z [N, 2], D [N, 2], e (int64)."""
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    M = zr.size - 1
    T = (zr, zi, zr + zr, zi + zi)
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    with np.errstate(all="ignore"):
        live = np.ones(N, bool)
        m = np.ones(N, np.int64)
        zpr, zpi = zr[1] + cr, zi[1] + ci
        dr, di = cr.copy(), ci.copy()
        if M == 1:
            dr, di = zpr.copy(), zpi.copy()
            m[:] = 0
        Dr, Di, e = np.ones(N), np.zeros(N), np.zeros(N, np.int64)
        best = zpr * zpr + zpi * zpi
        arg = np.zeros(N, np.int32)
        bz = np.stack([zpr, zpi], axis=1)
        bD = np.stack([Dr, Di], axis=1)
        be = e.copy()
        for i in range(1, int(mrd)):
            if not live.any():
                break
            # (every pixel is stepped; an escaped one is frozen by `live`: nothing of it is read again)
            nDr, nDi, ne = DD._dstep(zpr, zpi, Dr, Di, e, False)
            ndr, ndi, nm, nzr, nzi, mg = DD._zstep(T, dr, di, np.where(live, m, 0), cr, ci)
            esc = live & (mg >= 4.0)
            n[esc] = i
            live &= ~esc
            keep = live & (mg < best)
            best = np.where(keep, mg, best)
            arg = np.where(keep, i, arg).astype(np.int32)
            bz[keep, 0], bz[keep, 1] = nzr[keep], nzi[keep]
            bD[keep, 0], bD[keep, 1] = nDr[keep], nDi[keep]
            be = np.where(keep, ne, be)
            rdr, rdi, rm = DD._rebase(M, ndr, ndi, nm, nzr, nzi, mg)
            Dr, Di, e = np.where(live, nDr, Dr), np.where(live, nDi, Di), np.where(live, ne, e)
            dr, di, m = np.where(live, rdr, dr), np.where(live, rdi, di), np.where(live, rm, m)
            zpr, zpi = np.where(live, nzr, zpr), np.where(live, nzi, zpi)
    return {"n": n, "period": (arg + 1).astype(np.int32), "best": best, "z": bz, "D": bD, "e": be}


def model(orbit, view, mrd, window=None):
    """The states of a DeepView on a DeepOrbit with delta [N, 2] added, arrays flat in the window's image order."""
    zr, zi = orbit.table()
    dcr, dci = D.offsets(view, window)
    st = states(zr, zi, dcr, dci, mrd)
    st["delta"] = delta(st["z"][:, 0], st["z"][:, 1], st["D"][:, 0], st["D"][:, 1], st["e"], view.span_r)
    return st


def mpc_of(cr: Fraction, ci: Fraction):
    return mpmath.mpc(mpmath.mpf(cr.numerator) / cr.denominator, mpmath.mpf(ci.numerator) / ci.denominator)


def hp_argmin(centre, dc_r, dc_i, mrd, bits=TRUTH_BITS):
    """z_0 = c, z' = z^2 + c at `bits` bits from the exact c = C + dc, steps 1 .. mrd - 1 up to the escape: (the step of the
    smallest |z_n|^2 among the steps that did not escape -- the first one if equal --, the smallest and the second smallest
    |z_n|^2 as mpf)."""
    Cr, Ci = D.exact(centre[0]) + Fraction(float(dc_r)), D.exact(centre[1]) + Fraction(float(dc_i))
    with mpmath.workprec(bits):
        c = mpc_of(Cr, Ci)
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


def hp_newton(cr: Fraction, ci: Fraction, period: int, bits: int, rounds: int = 64):
    """Newton's method on Z_p(C) = 0 (Z_1 = C, D_1 = 1) from the seed, at `bits` bits: the root as an mpc."""
    with mpmath.workprec(bits):
        c = mpc_of(cr, ci)
        tiny = mpmath.ldexp(1, -(bits - 16))
        for _ in range(rounds):
            z, d = c, mpmath.mpc(1)
            for _ in range(period - 1):
                d = 2 * z * d + 1
                z = z * z + c
            step = z / d
            c = c - step
            if abs(step) <= tiny:
                return c
        raise AssertionError("mpmath Newton did not converge")


def hp_step_and_size(c, period: int):
    """At the mpc c, in the caller's precision: (the Newton step -Z_p / D_p, the size estimate 1 / (b l^2))."""
    z, d = c, mpmath.mpc(1)
    l, b = mpmath.mpc(1), mpmath.mpc(1)
    for _ in range(period - 1):
        l = l * 2 * z
        b = b + 1 / l
        d = 2 * z * d + 1
        z = z * z + c
    return -z / d, 1 / (b * l * l)


def hp_z(c, k: int):
    """Z_k at the mpc c (Z_1 = c)."""
    z = c
    for _ in range(k - 1):
        z = z * z + c
    return z
