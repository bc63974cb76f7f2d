"""The relief-shading contract of include/mbk.h ("Relief shading") in numpy, and its truth -- a helper module, not a conftest.
Written from the header's text, not from the C code.

    state   that of "Distance estimates" (tests/distance_model.py: states)
    normal  wr = fl(fl(zr dr) + fl(zi di)), wi = fl(fl(zi dr) - fl(zr di)), m = fl(fl(wr^2) + fl(wi^2));
            (0, 0) unless 0 < m < inf and n > 0; else s = fl(sqrt(m)), (fl(wr / s), fl(wi / s))
    shade   g = fl(fl(nx lx) + fl(ny ly)), t = fl(fl(g + h) / fl(1 + h)); q = 0 unless t > 0, 256 where t >= 1, else floor(256 t)
    colour  `inside` where the count is 0; else each of R, G, B of the MBK_RENDER_SMOOTH colour becomes (base q + 128) >> 8

numpy rounds every operation on its own and its division and square root are IEEE's, so everything here is the contract's bit
for bit.  hp_normal() runs the same recurrences with mpmath and returns the unit vector of z / d.
"""
from __future__ import annotations

import mpmath
import numpy as np

import distance_model as DM
import render_model as R


def normal(zr, zi, dr, di, n):
    """Arrays of final states -> normals [..., 2]."""
    zr, zi, dr, di = (np.asarray(a, np.float64) for a in (zr, zi, dr, di))
    with np.errstate(all="ignore"):
        p0 = zr * dr
        p1 = zi * di
        p2 = zi * dr
        p3 = zr * di
        wr = p0 + p1
        wi = p2 - p3
        r2 = wr * wr
        i2 = wi * wi
        m = r2 + i2
        s = np.sqrt(m)
        nx = wr / s
        ny = wi / s
    flat = ~(m > 0.0) | np.isinf(m) | (np.asarray(n) <= 0)
    return np.stack([np.where(flat, 0.0, nx), np.where(flat, 0.0, ny)], axis=-1)


def model(view, mrd, window=None):
    """(normals [nrows, ncols, 2], counts [nrows, ncols], states) of a view tuple (distance_model.axes)."""
    cr, ci = DM.axes(view, window)
    st = DM.states(np.tile(cr, ci.size), np.repeat(ci, cr.size), mrd)
    shape = (ci.size, cr.size)
    nrm = normal(st["zr"], st["zi"], st["dr"], st["di"], st["n"])
    return nrm.reshape(shape + (2,)), st["n"].reshape(shape), st


def point(cr, ci, mrd):
    """((nx, ny), n, extra) of one point."""
    st = DM.states([cr], [ci], mrd)
    nrm = normal(st["zr"], st["zi"], st["dr"], st["di"], st["n"])
    return (float(nrm[0, 0]), float(nrm[0, 1])), int(st["n"][0]), int(st["extra"][0])


def shade(nx, ny, lx, ly, h):
    """q per sample, int64."""
    assert np.isfinite([lx, ly, h]).all() and abs(lx) <= 1.0 and abs(ly) <= 1.0 and 0.0 <= h <= 2.0 ** 10
    nx = np.asarray(nx, np.float64)
    ny = np.asarray(ny, np.float64)
    lx, ly, h = np.float64(lx), np.float64(ly), np.float64(h)
    with np.errstate(all="ignore"):
        a = nx * lx
        b = ny * ly
        g = a + b
        num = g + h
        den = np.float64(1.0) + h
        t = num / den
    q = np.floor(np.where((t > 0.0) & (t < 1.0), t, 0.0) * 256.0).astype(np.int64)
    return np.where(t >= 1.0, 256, q)


def neutral(h):
    """The shade of a flat normal: floor(256 h / (1 + h)) in the contract's arithmetic."""
    return int(shade(0.0, 0.0, 0.0, 0.0, h))


def colour(palette, inside, scale, offset, lx, ly, h, counts, nu, normals):
    """Sample colours [..., 4], int64."""
    counts = np.asarray(counts, np.int32)
    normals = np.asarray(normals, np.float64)
    base = R.colour_smooth(palette, inside, scale, offset, counts, nu)
    q = shade(normals[..., 0], normals[..., 1], lx, ly, h)[..., None]
    lit = base.copy()
    lit[..., :3] = (base[..., :3] * q + 128) >> 8
    return np.where((counts == 0)[..., None], np.asarray(inside, np.int64), lit)


def render(palette, inside, scale, offset, lx, ly, h, s, counts, nu, normals):
    return R.resolve(colour(palette, inside, scale, offset, lx, ly, h, counts, nu, normals), s)


def hp_normal(cr, ci, n_model, extra_model, bits):
    """The same recurrences at `bits` from the same binary64 c, run for the model's count and run-on: (agrees, (nx, ny)).
    agrees: the high-precision orbit escapes at the model's n and runs on for the model's number of steps."""
    with mpmath.workprec(bits):
        c = mpmath.mpc(float(cr), float(ci))
        z, d = c, mpmath.mpc(1)
        n = 0
        for k in range(1, int(n_model) + 1):
            d = 2 * z * d + 1
            z = z * z + c
            if z.real * z.real + z.imag * z.imag >= 4:
                n = k
                break
        if n != n_model:
            return False, (float("nan"), float("nan"))
        extra = 0
        while extra < DM.RUN_ON and not (z.real * z.real + z.imag * z.imag >= DM.RADIUS2):
            d = 2 * z * d + 1
            z = z * z + c
            extra += 1
        if extra != extra_model:
            return False, (float("nan"), float("nan"))
        u = z / d
        u = u / abs(u)
        return True, (float(u.real), float(u.imag))
