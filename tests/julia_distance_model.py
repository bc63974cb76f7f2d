"""The distance-estimate contract of include/mbk.h ("Distance estimates for Julia views") in numpy, and its truth -- a helper
module, not a conftest.  Written from the header's text, not from the C code.

    z_0 = p (the pixel), d_0 = 1;  u = fl(fl(zr dr) - fl(zi di)), v = fl(fl(zr di) + fl(zi dr)), d' = (2u, 2v)      no "+ 1"
    z' = (fl(fl(fl(zr^2) - fl(zi^2)) + c_r), zi')   with  zi' = fl(fl(fl(2 zr) zi) + c_i)    where |c_i| < 2^-900 (literal)
                                                          zi' = fl(2 fl(zr zi) + c_i)         elsewhere (the fused form)
    n = first k with mag_k = fl(fl(zr^2) + fl(zi^2)) >= 4 (k = 1 .. mrd - 1), else 0
    n > 0: run on until mag >= 2^32 or 64 further steps, whatever mag does on the way
    de = fl(fl(sqrt(fl(mag / dmag))) fl(ln mag)), 0 if n = 0, 0 instead of NaN               distance_model.value, shared

numpy rounds every operation on its own, so the states (n, extra, z, d, mag, dmag) are the contract's bit for bit; only ln
can separate two implementations of de (distance_model.assert_states_agree / assert_expression_within, reused).

Pinned figures, by the rules of distance_model.py:
    J0   the output expression of the host (distance_value through mbk_julia_distance_host: glibc's ln) on the exact Julia
         (mag, dmag) pairs of SMALL_CASES against mpmath, in ulp(de): measured by
         tests/test_julia_distance.py::test_output_expression_against_mpmath, rounded up to two decimals; the test fails above
         it and fails if it is more than 0.1 above what it measures.  Measured 2.0018 at n = 1, mag = 37149473443.602585,
         dmag = 8582448776673.926 (c = i, sample 2985 of the 77 x 53 view).  The device gets J0 + 1 (ocml's ln).
    DERIVATIVE_REL   relative error of the model's de (binary64 orbit and derivative) against the same two recurrences at 256
         bits, on the escaped samples of DERIVATIVE_CASES whose count and run-on length agree: worst measured 1.314e-1
         (c = 0, sample 1020 of the 77 x 53 view: p = (-0.8, -0.6) as binary64, n = 53, de = 2.5e-16) -> 2e-1 (one digit,
         rounded up) x 4.  The figure is large because that sample lies within one ulp of the set: a rounding of the orbit is
         a displacement of the starting point by about an ulp of |p|, which is the whole of such a sample's distance.  The
         error is of that size everywhere, so the RELATIVE figure falls with the distance: per case the worst is 1.3e-1
         (c = 0; below 2e-14 apart from two samples on |p| = 1 + O(ulp)), 2.2e-12 (i), 5.9e-2 (-0.8 + 0.156i; de = 1.1e-16,
         n = 657), 1.1e-12 (-0.75), 4.7e-14 (-2), 7.8e-16 (2 + 1.5i), 1.5e-12 (-0.8 + 1e-301i).  At least 99 % of the escaped
         samples of each case take part (measured: one sample of c = -0.8 + 0.156i and one of c = -2 are left out).
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

import distance_model as D

PRECISION_BITS = D.PRECISION_BITS
RUN_ON = D.RUN_ON            # the constant pair of "Distance estimates"
RADIUS2 = D.RADIUS2
SAFE_IMAG_MIN = 2.0 ** -900  # |c_i| below this: the literal doubling ("Julia views")

J0 = 2.01
J_GPU = J0 + 1.0
DERIVATIVE_REL = 0.8

value = D.value
expression_true = D.expression_true
assert_states_agree = D.assert_states_agree
assert_expression_within = D.assert_expression_within
axes = D.axes

# (name, view, c, mrd, window): the cases the host twin and the GPU are held to on every sample
V77 = (-1.6, -1.2, 3.2, 2.4, 77, 53)
SMALL_CASES = [
    ("circle", V77, (0.0, 0.0), 300, None),
    ("dendrite", V77, (0.0, 1.0), 1000, None),
    ("dust", V77, (-0.8, 0.156), 1000, None),                 # max count 771
    ("neck", V77, (-0.75, 0.0), 1000, None),                  # c_i = 0: the literal loop; 1067 interior samples
    ("segment", V77, (-2.0, 0.0), 2000, None),                # literal, and |c|^2 = 4 takes the per-step rule
    ("far", V77, (2.0, 1.5), 100, None),                      # |c| > 2; run-on lengths 3 .. 5
    ("tiny-ci", V77, (-0.8, 1e-301), 1000, None),             # literal doubling by the 2^-900 rule
    ("critical", (-2.0, -2.0, 4.0, 4.0, 65, 65), (0.285, 0.01), 500, None),   # the centre pixel is z_0 = 0: +inf
    ("win-3-5-13-9", V77, (-0.8, 0.156), 1000, (3, 5, 13, 9)),
    ("win-76-52-1-1", V77, (-0.8, 0.156), 1000, (76, 52, 1, 1)),
    ("1x1", (0.7, 0.6, 0.0, 0.0, 1, 1), (-0.8, 0.156), 1000, None),
    ("2^499", (2.0 ** 499, -2.0 ** 499, 2.0 ** 498, 2.0 ** 499, 9, 5), (0.0, 1.0), 10, None),   # mag = inf: every de is +inf
]
# the cases whose derivative is held to 256 bits: the seven parameters on the 77 x 53 view, in which nothing overflows
DERIVATIVE_CASES = [c for c in SMALL_CASES if c[1] == V77 and c[4] is None]


def needs_literal(c_i) -> bool:
    return not (abs(float(c_i)) >= SAFE_IMAG_MIN)


def _step(zr, zi, dr, di, c_r, c_i, literal):
    p0 = zr * dr
    p1 = zi * di
    p2 = zr * di
    p3 = zi * dr
    u = p0 - p1
    v = p2 + p3
    a = zr * zr
    b = zi * zi
    t = a - b
    if literal:
        w = 2.0 * zr
        q = w * zi
    else:
        p = zr * zi
        q = 2.0 * p          # exact, so fl(q + c_i) is the fused result
    return t + c_r, q + c_i, 2.0 * u, 2.0 * v


_mag = D._mag


def states(zr0, zi0, c, mrd):
    """Flat arrays of starting points, one parameter c = (c_r, c_i) -> dict of flat arrays: n (int32), extra (run-on steps
    taken), zr, zi, dr, di, mag, dmag at the final state (where n = 0: after the mrd - 1 updates, or the initial state if no
    step ran)."""
    zr0 = np.asarray(zr0, np.float64).ravel()
    zi0 = np.asarray(zi0, np.float64).ravel()
    c_r, c_i = np.float64(c[0]), np.float64(c[1])
    literal = needs_literal(c_i)
    N = zr0.size
    out = {"n": np.zeros(N, np.int32), "extra": np.zeros(N, np.int32)}
    fin = {k: np.zeros(N, np.float64) for k in ("zr", "zi", "dr", "di")}
    fin["zr"][:], fin["zi"][:], fin["dr"][:] = zr0, zi0, 1.0
    idx = np.arange(N)
    zr, zi, dr, di = zr0.copy(), zi0.copy(), np.ones(N), np.zeros(N)
    with np.errstate(all="ignore"):
        for k in range(1, int(mrd)):
            if idx.size == 0:
                break
            zr, zi, dr, di = _step(zr, zi, dr, di, c_r, c_i, literal)
            esc = _mag(zr, zi) >= 4.0
            if esc.any():
                w = idx[esc]
                out["n"][w] = k
                fin["zr"][w], fin["zi"][w], fin["dr"][w], fin["di"][w] = zr[esc], zi[esc], dr[esc], di[esc]
                keep = ~esc
                idx, zr, zi, dr, di = idx[keep], zr[keep], zi[keep], dr[keep], di[keep]
        fin["zr"][idx], fin["zi"][idx], fin["dr"][idx], fin["di"][idx] = zr, zi, dr, di      # never escaped: the last state
        # the run-on of the escaped pixels: no `>= 4` test in it
        idx = np.flatnonzero(out["n"] > 0)
        zr, zi, dr, di = (fin[k][idx] for k in ("zr", "zi", "dr", "di"))
        for _ in range(RUN_ON):
            go = ~(_mag(zr, zi) >= RADIUS2)
            if not go.any():
                break
            nzr, nzi, ndr, ndi = _step(zr, zi, dr, di, c_r, c_i, literal)
            zr, zi, dr, di = (np.where(go, a, b) for a, b in ((nzr, zr), (nzi, zi), (ndr, dr), (ndi, di)))
            out["extra"][idx[go]] += 1
        fin["zr"][idx], fin["zi"][idx], fin["dr"][idx], fin["di"][idx] = zr, zi, dr, di
        out.update(fin)
        out["mag"] = _mag(fin["zr"], fin["zi"])
        out["dmag"] = _mag(fin["dr"], fin["di"])
    return out


def points(view, window=None):
    """The flat starting points (zr0, zi0) of a view tuple or a window of it, row-major."""
    re, im = axes(view, window)
    return np.tile(re, im.size), np.repeat(im, re.size)


def model(view, c, mrd, window=None):
    """(de, counts, states) of the Julia view of c, arrays [nrows, ncols] (states flat)."""
    re, im = axes(view, window)
    st = states(np.tile(re, im.size), np.repeat(im, re.size), c, mrd)
    shape = (im.size, re.size)
    return value(st["mag"], st["dmag"], st["n"]).reshape(shape), st["n"].reshape(shape), st


_MODELS = {}


def case_model(case):
    """model() of a SMALL_CASES entry, computed once and shared: treat it as read-only."""
    name, v, c, mrd, window = case
    if name not in _MODELS:
        _MODELS[name] = model(v, c, mrd, window)
    return _MODELS[name]


def hp_sample(z0r, z0i, c, n_model, extra_model):
    """The same two recurrences at PRECISION_BITS from the same binary64 z_0 and c, run for the model's count: (agrees, de as a
    float).  agrees: the high-precision orbit escapes at the model's n and runs on for the model's number of steps."""
    with mpmath.workprec(PRECISION_BITS):
        cc = mpmath.mpc(float(c[0]), float(c[1]))
        z, d = mpmath.mpc(float(z0r), float(z0i)), mpmath.mpc(1)
        n = 0
        for k in range(1, int(n_model) + 1):
            d = 2 * z * d
            z = z * z + cc
            if z.real * z.real + z.imag * z.imag >= 4:
                n = k
                break
        if n != n_model:
            return False, math.nan
        extra = 0
        while extra < RUN_ON and not (z.real * z.real + z.imag * z.imag >= RADIUS2):
            d = 2 * z * d
            z = z * z + cc
            extra += 1
        if extra != extra_model:
            return False, math.nan
        mag = z.real * z.real + z.imag * z.imag
        dmag = d.real * d.real + d.imag * d.imag
        if dmag == 0:
            return True, math.inf
        return True, float(mpmath.sqrt(mag / dmag) * mpmath.log(mag))
