"""The true interior distance estimate, for the tests -- a helper module, not a conftest.

The contract of an interior view (include/mbk.h, "Interior views") carries four derivatives of the p-fold map round the
cycle and stores de = (1 - |A|^2) / |F + E B / (1 - A)|.  tests/interior_model.py restates those recurrences, so it cannot say
whether they are the right ones.  What they are meant to compute is

    de = (1 - |lambda|^2) / |d lambda / dc|,        lambda(c) = the multiplier of the attracting cycle of z -> z^2 + c,

which needs none of them: lambda does not depend on the cycle point taken, and a quadratic map has at most one attracting
cycle.  truth() evaluates it with mpmath at 256 bits from the pixel's coordinate and a candidate period alone: a binary64
orbit to get near the cycle, Newton on f^p(z) - z to land on it, lambda = (f^p)'(z*), and d lambda / dc by central differences
of lambda(c +- 2^-70), the cycle continued from z* by Newton.  It also returns the exact minimal period of the cycle it
found, so that a contract period that is a multiple of the true one shows.  analytic() evaluates |F + E B / (1 - A)| with exact
recurrences at the same z*; tests/test_interior_truth.py asserts that the two agree to 1e-30, which is what says that the
contract's formula is the derivative of the multiplier.

The error measure.  The contract's de is the result of about 54 p rounded binary64 operations and ends in 1 - |A|^2, which
cancels as |lambda| -> 1, so its relative error grows like p / (1 - |lambda|^2):

    rel = |de - de_true| / de_true <= K * p * 2^-52 / (1 - |lambda|^2).

K0 is the worst K measured by tests/test_interior_truth.py over its three cases (the test prints K per case, fails if a pixel
exceeds K0 and fails if K0 is more than 10 % above what it measures).  The form fits: the worst K of the three cases (13, 20 and 69)
lie within a factor of six of each other although the pixels that set them have periods 1, 58 and 3, and no single pixel
dominates: the largest K of the 160 x 160 grid are 69 and 66 (a conjugate pair), 41, 34, 31 and 30, at periods 3, 2, 4, 2 and 10
(median 0.5, 99th percentile 12).  K0 has no device
margin: every operation of the contract is a correctly rounded binary64 one, and host, numpy and GPU are bit-identical.
"""
from __future__ import annotations

import mpmath
import numpy as np

import interior_model as M

PRECISION_BITS = 256
H_EXP = -70               # the finite difference's step, 2^H_EXP
NEWTON_MAX = 80
NEWTON_TOL_EXP = -230     # Newton stops at |dz| < 2^NEWTON_TOL_EXP
PERIOD_TOL_EXP = -200     # f^d(z*) == z* when they are within 2^PERIOD_TOL_EXP
EPS = 2.0 ** -52

# Measured by tests/test_interior_truth.py (numpy on x86-64; bit-identical to the host twin and the GPU), rounded up to two
# significant digits: 586 settled pixels of FULL64 (K 13.03), 50 of SEAHORSE (K 20.13, periods 27 / 29 / 58) and 4002 of GRID160
# (periods 1 to 29).  The worst pixel is in GRID160, in the period-3 component on the real axis:
K0 = 69.0   # measured 68.52 at c = (-1.7547169811320755, -0.009433962264151052), p = 3, |lambda| = 0.83773, rel = 1.53e-13

FULL64 = ((-2.0, -1.5, 3.0, 3.0, 64, 64), 1500)
# 0.02 wide around (-0.745, 0.11): periods 27, 29 and 58 (the view of tests/test_gpu_interior.py)
SEAHORSE = ((-0.755, 0.11 - 0.01 * 64 / 96, 0.02, 0.02 * 64 / 96, 96, 64), 2000)
GRID160 = ((-2.0, -1.5, 3.0, 3.0, 160, 160), 4096)

_MODEL = {}
_TRUTH = {}


def model_case(case):
    """(cr, ci, model dict) of a (view, mrd) case, flat arrays, computed once per session."""
    if case not in _MODEL:
        v, mrd = case
        xr, xi = M.axes(v)
        cr, ci = np.meshgrid(xr, xi)
        _MODEL[case] = (cr.ravel(), ci.ravel(), M.interior(cr, ci, mrd))
    return _MODEL[case]


def _cycle_map(z, c, p):
    """(f^p(z), (f^p)'(z)) in the working precision."""
    d = mpmath.mpc(1)
    for _ in range(p):
        d = 2 * z * d
        z = z * z + c
    return z, d


def _newton(z, c, p):
    """The fixed point of f^p near z and its multiplier, or None."""
    tol = mpmath.ldexp(mpmath.mpf(1), NEWTON_TOL_EXP)
    for _ in range(NEWTON_MAX):
        w, d = _cycle_map(z, c, p)
        dz = (w - z) / (d - 1)
        z = z - dz
        if abs(dz) < tol:
            return z, _cycle_map(z, c, p)[1]
    return None


def analytic(z, c, p):
    """|d lambda / dc| = |F + E B / (1 - A)| at the cycle point z of period p: A = dz, B = dc, E = dzz, F = dcz of the p-fold map,
    exact recurrences in the working precision."""
    A, B, E, F = mpmath.mpc(1), mpmath.mpc(0), mpmath.mpc(0), mpmath.mpc(0)
    for _ in range(p):
        F, E, B, A = 2 * (z * F + A * B), 2 * (A * A + z * E), 2 * z * B + 1, 2 * z * A
        z = z * z + c
    return abs(F + E * B / (1 - A))


def truth(cr, ci, p, warm, with_analytic=False):
    """(|lambda|, q, de_true) as binary64 / int / mpf for the pixel (cr, ci) and the candidate period p, or None if Newton
    does not converge: q is the exact minimal period of the cycle found.  with_analytic: a fourth element, the relative
    difference between the analytic |d lambda / dc| and the finite difference."""
    key = (float(cr), float(ci), int(p), int(warm))
    if key in _TRUTH and not with_analytic:
        return _TRUTH[key]
    p = int(p)
    zr, zi = float(cr), float(ci)
    for _ in range(int(warm)):                       # a plain binary64 orbit: any point near the cycle will do
        zr, zi = zr * zr - zi * zi + float(cr), 2.0 * zr * zi + float(ci)
    with mpmath.workprec(PRECISION_BITS):
        c = mpmath.mpc(float(cr), float(ci))
        got = _newton(mpmath.mpc(zr, zi), c, p)
        if got is None:
            _TRUTH[key] = None
            return None
        z, lam = got
        tol = mpmath.ldexp(mpmath.mpf(1), PERIOD_TOL_EXP)
        q, y = 0, z
        for d in range(1, p + 1):
            y = y * y + c
            if p % d == 0 and abs(y - z) < tol:
                q = d
                break
        h = mpmath.ldexp(mpmath.mpf(1), H_EXP)
        plus, minus = _newton(z, c + h, p), _newton(z, c - h, p)
        if q == 0 or plus is None or minus is None:
            _TRUTH[key] = None
            return None
        dlam = abs((plus[1] - minus[1]) / (2 * h))
        de = (1 - abs(lam) ** 2) / dlam
        out = (float(abs(lam)), q, de)
        _TRUTH[key] = out
        if with_analytic:
            return out + (float(abs(analytic(z, c, p) - dlam) / dlam),)
        return out


def measure(cr, ci, period, de, warm, what, with_analytic=False):
    """Hold the (period, de) of every settled pixel (period > 0) of flat arrays to truth().  Returns a dict: settled, the pixels
    that did not converge, whose exact period differs and whose |lambda| >= 1 (lists of flat indices), K = the worst
    rel (1 - |lambda|^2) / (p 2^-52) with the pixel that sets it, the worst rel, and worst_analytic."""
    cr, ci = np.asarray(cr, np.float64).ravel(), np.asarray(ci, np.float64).ravel()
    period, de = np.asarray(period).ravel(), np.asarray(de, np.float64).ravel()
    out = {"settled": 0, "no_newton": [], "wrong_period": [], "not_attracting": [], "K": 0.0, "K_at": None, "rel": 0.0,
           "worst_analytic": 0.0}
    with mpmath.workprec(PRECISION_BITS):
        for i in np.flatnonzero(period > 0):
            out["settled"] += 1
            t = truth(cr[i], ci[i], period[i], warm, with_analytic)
            if t is None:
                out["no_newton"].append(int(i))
                continue
            lam, q, de_true = t[:3]
            if with_analytic:
                out["worst_analytic"] = max(out["worst_analytic"], t[3])
            if q != period[i]:
                out["wrong_period"].append(int(i))
            if not lam < 1.0:
                out["not_attracting"].append(int(i))
                continue
            rel = float(abs(mpmath.mpf(float(de[i])) - de_true) / de_true)
            k = rel * float(1 - mpmath.mpf(lam) ** 2) / (int(period[i]) * EPS)
            out["rel"] = max(out["rel"], rel)
            if k > out["K"]:
                out["K"], out["K_at"] = k, (float(cr[i]), float(ci[i]), int(period[i]), lam, rel)
    print(f"{what}: {out['settled']} settled pixels, K {out['K']:.2f} at (cr, ci, p, |lambda|, rel) = {out['K_at']}, worst rel "
          f"{out['rel']:.3e}" + (f", analytic against finite difference {out['worst_analytic']:.1e}" if with_analytic else ""))
    return out


def assert_truth(cr, ci, period, de, warm, what, with_analytic=False):
    """measure(), then the conditions, every one with a cap of zero: every settled pixel converges, has the exact minimal
    period the arrays say, is attracting, and lies within K0.  Returns the figures."""
    w = measure(cr, ci, period, de, warm, what, with_analytic)
    assert w["settled"] > 0, what
    assert not w["no_newton"], (what, "Newton did not converge", w["no_newton"][:5])
    assert not w["wrong_period"], (what, "not the minimal period", w["wrong_period"][:5])
    assert not w["not_attracting"], (what, "|lambda| >= 1", w["not_attracting"][:5])
    assert w["K"] <= K0, (what, w["K"], w["K_at"])
    return w
