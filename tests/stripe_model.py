"""The stripe-average contract of include/mbk.h ("Stripe-average colouring") in numpy, and its truth -- a helper module, not a
conftest.  Written from the header's text, not from the C code.

    orbit   z_0 = c, the reference's recurrence, n = first k with mag_k >= 4 (k = 1 .. mrd - 1), else 0; n > 0 runs on until
            mag >= 2^32 or 64 further steps; N = n + run-on steps
    term    t_k = 0.5 unless 0 < mag_k < inf; else r = fl(sqrt(mag_k)), u = (fl(zr / r), fl(zi / r)), p = u, s - 1 times
            p <- (fl(fl(p.r u.r) - fl(p.i u.i)), fl(fl(p.r u.i) + fl(p.i u.r))), t_k = fl(0.5 + fl(0.5 p.i))
    sum     S adds t_k for k = skip + 1 .. N in ascending order; cnt = max(0, N - skip); t_last = t_N if cnt > 0 else 0
    value   0 if n = 0; 0.5 if cnt = 0; S if cnt = 1; else a1 = fl(S / cnt), a0 = fl(fl(S - t_last) / (cnt - 1)),
            d = fl(1 - fl(log2(fl(fl(ln mag_N) / LB)))) clamped to [0, 1] (0 for a NaN), v = fl(a0 + fl(fl(a1 - a0) d))
    shade   w = fl(0.5 + fl(gain fl(v - 0.5))) clamped to [0, 1], t = fl(lo + fl(fl(1 - lo) w)), q = floor(256 t), 256 where t >= 1
    colour  `inside` where the count is 0; else each of R, G, B of the MBK_RENDER_SMOOTH colour becomes (base q + 128) >> 8

numpy rounds every operation on its own and its division and square root are IEEE's, so the states here are the contract's bit
for bit; only ln and log2 can separate two implementations of v.  value_true() evaluates the value expression with mpmath on
the exact state, hp_value() runs the same recurrences with the true sin(s arg z) at high precision.
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

import distance_model as DM
import render_model as R

RUN_ON = DM.RUN_ON
RADIUS2 = DM.RADIUS2
LB = 32.0 * math.log(2.0)          # the binary64 nearest 32 ln 2: a power of two times the nearest of ln 2
assert LB == 32.0 * float.fromhex("0x1.62e42fefa39efp-1")
TRUTH_BITS = 384

# Measured by tests/test_stripe.py::test_value_against_the_correctly_rounded_value (glibc's libm on x86-64): the largest error of
# mbk_stripe_value_host against the value expression in mpmath at the exact state, in ulp(v), over the escaped pixels of the
# seahorse view at densities 1, 5, 16; rounded up to two decimals.  The test prints the figure, fails if a pixel exceeds it and
# fails if it is more than 0.1 above what it measures.  The device is allowed one ulp more (ocml's ln and log2 against
# glibc's, as for de in distance_model.py).
# Measured 1.4470 at density 5, skip 3.
MEASURED_VALUE_ULPS_HOST = 1.45
VALUE_ULPS_GPU = MEASURED_VALUE_ULPS_HOST + 1.0

# |model v - true v| per (point, density), measured by tests/test_stripe.py::test_model_against_mpmath at mrd 5000 with the true
# sin(s arg z_k) at TRUTH_BITS; the test allows 4 x the figure: rounding in z is amplified near the boundary and the constant is
# a record, not a bound.
TRUTH_POINTS = [((0.37, 0.6), 17), ((-1.75, 0.02), 12), ((-0.7436438860371587, 0.1318259043091895), 1194)]
TRUTH_DENSITIES = (1, 5, 16)
MEASURED_TRUTH = {
    ((0.37, 0.6), 1): 2.23e-16, ((0.37, 0.6), 5): 1.34e-15, ((0.37, 0.6), 16): 2.45e-15,
    ((-1.75, 0.02), 1): 1.92e-14, ((-1.75, 0.02), 5): 3.50e-14, ((-1.75, 0.02), 16): 1.61e-13,
    ((-0.7436438860371587, 0.1318259043091895), 1): 7.57e-7, ((-0.7436438860371587, 0.1318259043091895), 5): 1.02e-6,
    ((-0.7436438860371587, 0.1318259043091895), 16): 6.23e-6,
}


def _step(zr, zi, cr, ci):
    a = zr * zr
    b = zi * zi
    t = a - b
    w = 2.0 * zr
    q = w * zi
    return t + cr, q + ci


def _mag(x, y):
    a = x * x
    b = y * y
    return a + b


def term(zr, zi, mag, s):
    """t_k of arrays of points."""
    zr, zi, mag = (np.asarray(a, np.float64) for a in (zr, zi, mag))
    with np.errstate(all="ignore"):
        r = np.sqrt(mag)
        ur = zr / r
        ui = zi / r
        pr, pi = ur, ui
        for _ in range(int(s) - 1):
            m0 = pr * ur
            m1 = pi * ui
            m2 = pr * ui
            m3 = pi * ur
            pr, pi = m0 - m1, m2 + m3
        h = 0.5 * pi
        t = 0.5 + h
    return np.where((mag > 0.0) & ~np.isinf(mag), t, 0.5)


def states(cr, ci, mrd, density, skip):
    """Flat arrays cr, ci -> dict of flat arrays: n, N, cnt (int32), S, t_last, mag (float64); all zero where n = 0."""
    assert 1 <= density <= 16 and 0 <= skip < 2 ** 31
    cr = np.asarray(cr, np.float64).ravel()
    ci = np.asarray(ci, np.float64).ravel()
    P = cr.size
    out = {k: np.zeros(P, np.int32) for k in ("n", "N", "cnt")}
    out.update({k: np.zeros(P, np.float64) for k in ("S", "t_last", "mag")})
    fz = {k: np.zeros(P, np.float64) for k in ("zr", "zi")}
    idx = np.arange(P)
    zr, zi, c_r, c_i = cr.copy(), ci.copy(), cr.copy(), ci.copy()
    S, tl = np.zeros(P), np.zeros(P)
    with np.errstate(all="ignore"):
        for k in range(1, int(mrd)):
            if idx.size == 0:
                break
            zr, zi = _step(zr, zi, c_r, c_i)
            mag = _mag(zr, zi)
            if k > skip:
                tl = term(zr, zi, mag, density)
                S = S + tl
            esc = mag >= 4.0
            if esc.any():
                w = idx[esc]
                out["n"][w] = k
                out["S"][w], out["t_last"][w], out["mag"][w] = S[esc], tl[esc], mag[esc]
                fz["zr"][w], fz["zi"][w] = zr[esc], zi[esc]
                keep = ~esc
                idx, zr, zi, c_r, c_i, S, tl = (a[keep] for a in (idx, zr, zi, c_r, c_i, S, tl))
        # the run-on of the escaped pixels
        idx = np.flatnonzero(out["n"] > 0)
        zr, zi, c_r, c_i = fz["zr"][idx], fz["zi"][idx], cr[idx], ci[idx]
        S, tl, mag = out["S"][idx], out["t_last"][idx], out["mag"][idx]
        N = out["n"][idx].astype(np.int64)
        for _ in range(RUN_ON):
            go = ~(mag >= RADIUS2)
            if not go.any():
                break
            nzr, nzi = _step(zr, zi, c_r, c_i)
            nmag = _mag(nzr, nzi)
            N = N + go
            add = go & (N > skip)
            nt = term(nzr, nzi, nmag, density)
            S = np.where(add, S + nt, S)
            tl = np.where(add, nt, tl)
            zr, zi, mag = np.where(go, nzr, zr), np.where(go, nzi, zi), np.where(go, nmag, mag)
        out["S"][idx], out["t_last"][idx], out["mag"][idx] = S, tl, mag
        out["N"][idx] = N
        out["cnt"][idx] = np.maximum(0, N - skip)
    return out


def value(S, t_last, cnt, mag, n, ln=None, lg=None):
    """The value expression on arrays; ln, lg: functions in place of numpy's log and log2."""
    S, t_last, mag = (np.asarray(a, np.float64) for a in (S, t_last, mag))
    cnt = np.asarray(cnt, np.int64)
    n = np.asarray(n)
    with np.errstate(all="ignore"):
        a1 = S / np.maximum(cnt, 1).astype(np.float64)
        rest = S - t_last
        a0 = rest / np.maximum(cnt - 1, 1).astype(np.float64)
        l = (ln or np.log)(mag)
        q = l / np.float64(LB)
        g = (lg or np.log2)(q)
        d = 1.0 - g
        d = np.where(d >= 0.0, d, 0.0)
        d = np.where(d > 1.0, 1.0, d)
        diff = a1 - a0
        w = diff * d
        v = a0 + w
    v = np.where(cnt == 1, S, v)
    v = np.where(cnt <= 0, 0.5, v)
    return np.where(n > 0, v, 0.0)


def model(view, mrd, density, skip, window=None):
    """(states (dict of arrays [nrows, ncols]), counts [nrows, ncols], v [nrows, ncols]) of a view tuple."""
    cr, ci = DM.axes(view, window)
    st = states(np.tile(cr, ci.size), np.repeat(ci, cr.size), mrd, density, skip)
    shape = (ci.size, cr.size)
    st = {k: a.reshape(shape) for k, a in st.items()}
    return st, st["n"], value(st["S"], st["t_last"], st["cnt"], st["mag"], st["n"])


def point(cr, ci, mrd, density, skip=0):
    """The state of one point as a dict of Python numbers, with its value "v"."""
    st = states([cr], [ci], mrd, density, skip)
    out = {k: (int(a[0]) if a.dtype == np.int32 else float(a[0])) for k, a in st.items()}
    out["v"] = float(value(st["S"], st["t_last"], st["cnt"], st["mag"], st["n"])[0])
    return out


def value_true(S, t_last, cnt, mag, n):
    """The value expression on the exact doubles of one state in mpmath (256 bits): an mpf.  The special cases of the header."""
    if int(n) <= 0:
        return mpmath.mpf(0)
    if int(cnt) <= 0:
        return mpmath.mpf(0.5)
    if int(cnt) == 1:
        return mpmath.mpf(float(S))
    with mpmath.workprec(256):
        a1 = mpmath.mpf(float(S)) / int(cnt)
        a0 = (mpmath.mpf(float(S)) - mpmath.mpf(float(t_last))) / (int(cnt) - 1)
        if math.isnan(mag) or math.isinf(mag) or not mag > 0.0:
            d = mpmath.mpf(0)
        else:
            q = mpmath.log(mpmath.mpf(float(mag))) / mpmath.mpf(LB)
            d = 1 - mpmath.log(q, 2) if q > 0 else mpmath.mpf(0)
            d = min(max(d, mpmath.mpf(0)), mpmath.mpf(1))
        return a0 + (a1 - a0) * d


def value_err_ulps(got, st):
    """Error of `got` (flat) against value_true at the exact states, in ulp(v) of the truth's nearest double, per element;
    0 for the pixels whose value involves no logarithm when got equals it exactly (nan otherwise)."""
    got = np.asarray(got, np.float64).ravel()
    S, tl, cnt, mag, n = (np.asarray(st[k]).ravel() for k in ("S", "t_last", "cnt", "mag", "n"))
    out = np.zeros(got.size)
    with mpmath.workprec(256):
        for i in range(got.size):
            v = value_true(S[i], tl[i], cnt[i], mag[i], n[i])
            if n[i] <= 0 or cnt[i] <= 1:
                out[i] = 0.0 if got[i] == float(v) else math.nan
                continue
            out[i] = float(abs(mpmath.mpf(float(got[i])) - v) / mpmath.mpf(float(np.spacing(abs(float(v))))))
    return out


def hp_value(cr, ci, n_model, N_model, density, skip, bits=TRUTH_BITS):
    """The same recurrences at `bits` from the same binary64 c with the true sin(s arg z_k): (agrees, v as a float).
    agrees: the high-precision orbit escapes at the model's n and its run-on ends at the model's N."""
    with mpmath.workprec(bits):
        c = mpmath.mpc(float(cr), float(ci))
        z = c
        n = 0
        terms = []
        for k in range(1, int(n_model) + 1):
            z = z * z + c
            terms.append((1 + mpmath.sin(density * mpmath.arg(z))) / 2)
            if z.real * z.real + z.imag * z.imag >= 4:
                n = k
                break
        if n != n_model:
            return False, math.nan
        N = n
        while N - n < RUN_ON and not (z.real * z.real + z.imag * z.imag >= RADIUS2):
            z = z * z + c
            terms.append((1 + mpmath.sin(density * mpmath.arg(z))) / 2)
            N += 1
        if N != N_model:
            return False, math.nan
        used = terms[skip:]
        cnt = len(used)
        if cnt == 0:
            return True, 0.5
        if cnt == 1:
            return True, float(used[0])
        a1 = mpmath.fsum(used) / cnt
        a0 = mpmath.fsum(used[:-1]) / (cnt - 1)
        mag = z.real * z.real + z.imag * z.imag
        d = 1 - mpmath.log(mpmath.log(mag) / (32 * mpmath.log(2)), 2)
        d = min(max(d, mpmath.mpf(0)), mpmath.mpf(1))
        return True, float(a0 + (a1 - a0) * d)


def shade(v, lo, gain):
    """q per sample, int64."""
    assert np.isfinite([lo, gain]).all() and 0.0 <= lo <= 1.0 and 0.0 <= gain <= 2.0 ** 10
    v = np.asarray(v, np.float64)
    lo, gain = np.float64(lo), np.float64(gain)
    with np.errstate(all="ignore"):
        c = v - 0.5
        g = gain * c
        w = 0.5 + g
        w = np.where(w >= 0.0, w, 0.0)
        w = np.where(w > 1.0, 1.0, w)
        span = np.float64(1.0) - lo
        m = span * w
        t = lo + m
    q = np.floor(np.where((t > 0.0) & (t < 1.0), t, 0.0) * 256.0).astype(np.int64)
    return np.where(t >= 1.0, 256, q)


def neutral(lo):
    """The shade at gain 0 (w = 0.5 whatever v)."""
    return int(shade(0.5, lo, 0.0))


def colour(palette, inside, scale, offset, lo, gain, counts, nu, v):
    """Sample colours [..., 4], int64."""
    counts = np.asarray(counts, np.int32)
    base = R.colour_smooth(palette, inside, scale, offset, counts, nu)
    q = shade(v, lo, gain)[..., None]
    lit = base.copy()
    lit[..., :3] = (base[..., :3] * q + 128) >> 8
    return np.where((counts == 0)[..., None], np.asarray(inside, np.int64), lit)


def render(palette, inside, scale, offset, lo, gain, s, counts, nu, v):
    return R.resolve(colour(palette, inside, scale, offset, lo, gain, counts, nu, v), s)
