"""The true value of the continuous escape-time formula, for the tests -- a helper module, not a conftest.

    nu = n + 1 - log2(0.5 * ln mag)      n = escape index, mag = |z_n|^2, the binary64 value that tripped `>= 4`

The kernels, the C oracle and tests/deep_model.py each evaluate this with their own logarithms (ocml, glibc, numpy).
nu_true() evaluates it with mpmath at 256 bits on the exact double `mag`, so that all of them can be held to the
correctly rounded result instead of to each other.

The error measure: err_abs = |got - nu|, err_ulps = err_abs / ulp(nu_true), ulp() of the nearest double.  The bound
has two terms,

    err_abs <= A * ulp(nu) + B * 2^-52,

because the error of L = log2(0.5 ln mag) is absolute (|L| <= ~9.5 for every finite mag >= 4, whatever n is) while
ulp(nu) goes to 0 where nu does (n = 1 and mag near e^8; mag reaches that size only when |c| > 2, at n <= 9).  The
two constants are measured on separate sets, so that each pixel is covered by one term alone:

    A0 = worst err_ulps      over the pixels with |nu| >= 1   (ulp(nu) >= 2^-52)
    B0 = worst err_abs/2^-52 over the pixels with |nu| <  1   (ulp(nu) <  2^-52: counting in ulps says nothing)

of the CPU reference (the libm oracle) over every CPU case of tests/test_smooth_truth.py.  The GPU is allowed
A = A0 + 1 and B = B0 + 2: ocml and glibc both aim at <= 1 ulp per call, there are two calls, each of which moves L by
about its own ulp (<= ~2^-52 while |L| < 2, the pixels of any ordinary view), and the last subtraction rounds by half
an ulp(nu) on either side.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

PRECISION_BITS = 256

# Measured by tests/test_smooth_truth.py over 42 cases and 113 061 escaped pixels (glibc's libm on x86-64; the test
# prints the figures, fails if a case exceeds them, and fails if they are more than 0.1 above what it measures), rounded
# up to two decimals.  Both worst pixels are in the "far" view (|c| from 2.2 to 74), at n = 1:
A0 = 1.57     # ulp(nu), |nu| >= 1: measured 1.5698 at mag = 11337031.25       (nu = -1.02, L = log2(0.5 ln mag) = 3.02)
B0 = 1.38     # 2^-52,   |nu| <  1: measured 1.3786 at mag = 75820.85571289062 (nu = -0.49, L = 2.49)
A_GPU = A0 + 1.0
B_GPU = B0 + 2.0
EPS = 2.0 ** -52


def nu_true(n: int, mag: float):
    """(nearest double, mpf at PRECISION_BITS) of n + 1 - log2(0.5 ln mag).  n == 0 (never escaped): 0.  mag == +inf
    (|z_n|^2 overflowed binary64): -inf, the limit of the formula and what IEEE logarithms give."""
    n = int(n)
    mag = float(mag)
    if n == 0:
        return 0.0, mpmath.mpf(0)
    if math.isnan(mag) or mag < 4.0:
        raise ValueError(f"mag {mag!r} is no escaping |z|^2")
    if math.isinf(mag):
        return -math.inf, mpmath.mpf("-inf")
    with mpmath.workprec(PRECISION_BITS):
        m = mpmath.mpf(mag)                         # exact: a double is a 53-bit mpf
        v = n + 1 - mpmath.log(mpmath.log(m) / 2, 2)
        return float(v), v                           # float() rounds to nearest even


def nu_true_array(counts, mag):
    """(nearest float64 array, rest float64 array) with nu = nearest + rest to ~1e-30: err() needs both."""
    counts = np.asarray(counts)
    mag = np.asarray(mag, np.float64)
    near = np.zeros(counts.shape, np.float64)
    rest = np.zeros(counts.shape, np.float64)
    nf, rf, cf, mf = near.reshape(-1), rest.reshape(-1), counts.reshape(-1), mag.reshape(-1)
    with mpmath.workprec(PRECISION_BITS):
        for i in np.flatnonzero(cf > 0):
            d, v = nu_true(cf[i], mf[i])
            nf[i] = d
            if math.isfinite(d):
                rf[i] = float(v - mpmath.mpf(d))
    return near, rest


def ulp(x):
    """Spacing of binary64 at |x| (numpy's: the gap to the next double away from zero)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)))


def err(got, near, rest):
    """(err_abs, err_ulps) of `got` against nu = near + rest.  got - near is exact when they are within a factor 2
    (Sterbenz).  Infinite truths: 0 if got is the same infinity, inf otherwise; a NaN in got gives inf."""
    got = np.asarray(got, np.float64)
    near = np.asarray(near, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs((got - near) - rest)
    same_inf = np.isinf(near) & (got == near)
    e = np.where(same_inf, 0.0, e)
    e = np.where(np.isnan(e), np.inf, e)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(np.isinf(near), 1.0, ulp(np.where(np.isinf(near), 1.0, near)))
        return e, e / u


def bound(near, A=A_GPU, B=B_GPU):
    """A ulp(nu) + B 2^-52 per pixel (0 where the truth is infinite or the pixel never escaped: equality)."""
    near = np.asarray(near, np.float64)
    fin = np.isfinite(near) & (near != 0.0)
    return np.where(fin, A * ulp(np.where(fin, near, 1.0)) + B * EPS, 0.0)


def worst(got, counts, mag, truth=None):
    """Figures of `got` against the truth on every escaped pixel: dict with A (worst err_ulps where |nu| >= 1), B (worst
    err_abs / 2^-52 where |nu| < 1), err_abs, where each occurred (flat index, n, mag), and the truth (near, rest), which
    a caller that compares several results on the same pixels passes back in as `truth`."""
    counts = np.asarray(counts).reshape(-1)
    mag = np.asarray(mag, np.float64).reshape(-1)
    got = np.asarray(got, np.float64).reshape(-1)
    near, rest = truth if truth is not None else nu_true_array(counts, mag)
    e, eu = err(got, near, rest)
    esc = counts > 0
    big = esc & (np.abs(near) >= 1.0)
    small = esc & (np.abs(near) < 1.0)
    out = {"n_escaped": int(esc.sum()), "A": 0.0, "B": 0.0, "err_abs": 0.0, "A_at": None, "B_at": None}
    if big.any():
        i = int(np.flatnonzero(big)[np.argmax(eu[big])])
        out["A"], out["A_at"] = float(eu[i]), (i, int(counts[i]), float(mag[i]))
    if small.any():
        i = int(np.flatnonzero(small)[np.argmax(e[small])])
        out["B"], out["B_at"] = float(e[i] / EPS), (i, int(counts[i]), float(mag[i]))
    fin = esc & np.isfinite(near)
    if fin.any():
        out["err_abs"] = float(e[fin].max())
    out["near"], out["rest"], out["err"] = near, rest, e
    return out


def assert_within(got, counts, mag, what, A=A_GPU, B=B_GPU, truth=None):
    """Every escaped pixel of `got` within A ulp(nu) + B 2^-52 of the truth (the same infinity where the truth is
    infinite), exactly 0 where the count is 0, no NaN.  Prints the figures first and returns them."""
    got = np.asarray(got, np.float64).reshape(-1)
    counts = np.asarray(counts).reshape(-1)
    mag = np.asarray(mag, np.float64).reshape(-1)
    w = worst(got, counts, mag, truth)
    print(f"{what}: {w['n_escaped']} escaped, A {w['A']:.3f} ulp at {w['A_at']}, B {w['B']:.3f} x 2^-52 at {w['B_at']}, "
          f"err_abs {w['err_abs']:.3e}")
    assert not np.isnan(got).any(), what
    assert (got[counts == 0] == 0.0).all(), what
    bad = (counts > 0) & ~(w["err"] <= bound(w["near"], A, B))
    assert not bad.any(), (what, int(bad.sum()), [(int(i), int(counts[i]), float(mag[i]), float(got[i]), float(w["near"][i]))
                                                   for i in np.flatnonzero(bad)[:5]])
    return w


def pair_bound(near_or_values, A1=A_GPU, B1=B_GPU, A2=A0, B2=B0):
    """Bound on |gpu - oracle| for whole arrays (triangle inequality): the sum of the two sides' bounds, evaluated at
    ulp of the oracle's values."""
    v = np.abs(np.asarray(near_or_values, np.float64))
    fin = np.isfinite(v) & (v != 0.0)
    u = ulp(np.where(fin, v, 1.0) * (1.0 + 2.0 ** -48))      # the truth may lie just across a power of two
    return np.where(fin, (A1 + A2) * u + (B1 + B2) * EPS, 0.0)


def assert_pair(gpu_nu, oracle_nu, counts, what):
    """GPU against the libm oracle on a whole array: identical zeros and infinities, no NaN, finite values within
    pair_bound."""
    gpu_nu = np.asarray(gpu_nu, np.float64)
    oracle_nu = np.asarray(oracle_nu, np.float64)
    assert not np.isnan(gpu_nu).any(), what
    assert np.array_equal(gpu_nu == 0.0, np.asarray(counts) == 0), what
    assert np.array_equal(np.isinf(gpu_nu), np.isinf(oracle_nu)), what
    fin = np.isfinite(oracle_nu)
    assert np.array_equal(gpu_nu[~fin], oracle_nu[~fin]), what
    d = np.abs(gpu_nu[fin] - oracle_nu[fin])
    b = pair_bound(oracle_nu[fin])
    print(f"{what}: worst |gpu - oracle| {float(d.max()) if d.size else 0.0:.3e}")
    assert (d <= b).all(), (what, float(d.max()), int((d > b).sum()))


def cfg5_sample(counts, mag, seed=5, n_random=20000, n_extreme=1000):
    """Flat indices of the cfg5 truth sample: n_random seeded escaped pixels, the n_extreme with the largest mag and
    the n_extreme with the smallest."""
    cf = np.asarray(counts).reshape(-1)
    mf = np.asarray(mag, np.float64).reshape(-1)
    esc = np.flatnonzero(cf > 0)
    pick = np.random.RandomState(seed).choice(esc, n_random, replace=False)
    order = np.argsort(mf[esc], kind="stable")
    return np.unique(np.concatenate([pick, esc[order[:n_extreme]], esc[order[-n_extreme:]]]))


# The plain views of the smooth tests, CPU (oracle against the truth) and GPU (kernels against the truth) alike:
# (name, (start_r, start_i, range_r, range_i, width, height), mrd, window or None).
RAGGED = [(1, 1), (1, 64), (64, 1), (7, 9), (8, 8), (9, 8), (31, 33), (32, 8), (33, 9), (65, 17)]
WINDOWS = [(0, 0, 77, 53), (5, 7, 40, 30), (76, 52, 1, 1), (0, 10, 77, 3), (13, 0, 1, 53)]
RING = ("ring", (-2.0, -2.0, 4.0, 4.0, 65, 33), 40, None)          # |c| = 2 on its edges; c = -2 + 0i at row 16, col 0
HUGE = ("huge", (1e76, 0.0, 1.9e77, 1e76, 64, 8), 10, None)        # mag ~ c^4 overflows binary64 near c = 1.16e77
TWO_499 = ("2^499", (2.0 ** 499, -2.0 ** 499, 2.0 ** 498, 2.0 ** 499, 9, 5), 10, None)     # mag = inf everywhere
SMALL_CASES = (
    [("%dx%d" % wh, (-0.9, 0.05, 0.6, 0.45) + wh, 200, None) for wh in RAGGED]
    + [("win-%d-%d-%d-%d" % w, (-1.3, -0.4, 1.1, 0.9, 77, 53), 333, w) for w in WINDOWS]
    + [("step0", (-0.75, 0.1, 0.0, 0.0, 5, 4), 100, None),
       ("step0-i", (0.3, 0.0, 1e-3, 5e-324, 9, 6), 100, None),
       ("tiny-i", (-1.8, 1e-310, 2.2, 3e-310, 96, 24), 500, None),
       RING,
       ("far", (2.0, 1.0, 60.0, 40.0, 33, 17), 10, None),           # |c| from 2.2 to 74: nu passes through 0 at n = 1
       HUGE, TWO_499])
CFG5 = ((-2.0, -1.5, 3.0, 3.0, 4096, 4096), 5000)

# Deep views whose smooth output is held to the truth: (centre, span_r, (width, height), span_i or None, mrd, window).
SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
DEEP_CASES = [
    (SEAHORSE, 1e-8, (128, 128), None, 5000, None),
    (SEAHORSE, 1e-20, (128, 96), None, 30000, None),
    (("0", "1"), 1e-60, (64, 64), None, 5000, None),
    (("0", "1"), 1e-200, (256, 256), None, 5000, None),
    (("1e-21", "1"), 1e-20, (100, 70), None, 5000, None),
    (("-2", "0"), 1e-60, (40, 24), None, 200, None),               # M == 1, every pixel retires at count 1
    (("1e-21", "1"), 1e-20, (90, 60), None, 5000, (5, 7, 70, 41)),
    (("0", "1"), 2.0 ** -960, (24, 20), 2.0 ** -960, 3000, None),  # the deepest span
    (("-0.5", "0"), 4.0, (64, 56), None, 400, None),               # the widest
    (("-2", "0"), 1.0, (64, 48), None, 2000, None),                # M == 1: mag comes from the rebased state
]


def deep_model_case(case):
    """(orbit, view, mrd, window, model counts, model mag) of a DEEP_CASES entry, arrays [rows, cols] of the window."""
    import deep_model as D
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    centre, span, size, span_i, mrd, window = case
    orbit = DeepOrbit(*centre, mrd, min_span=min(span, span_i or span))
    view = DeepView(span, size[0], size[1], span_i)
    zr, zi = orbit.table()
    dr, di = D.offsets(view, window)
    c, mag = D.model_counts(zr, zi, dr, di, mrd)
    rows = window[3] if window else view.height
    return orbit, view, mrd, window, c.reshape(rows, -1), mag.reshape(rows, -1)


_CFG5 = {}


def cfg5_oracle(oracle):
    """(nu, counts, mag) of cfg5 from the C oracle, computed once per session and shared by the tests that need it."""
    if "v" not in _CFG5:
        _CFG5["v"] = oracle.view_smooth_mag(*CFG5[0], CFG5[1])
    return _CFG5["v"]
