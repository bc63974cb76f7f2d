"""The distance-estimate contract of include/mbk.h ("Distance estimates") in numpy, and its truth -- a helper module, not a
conftest.  Written from the header's text, not from the C code.

    z_0 = c, d_0 = 1;  u = fl(fl(zr dr) - fl(zi di)), v = fl(fl(zr di) + fl(zi dr)), d' = (fl(2u + 1), 2v),
    z' = (fl(fl(fl(zr^2) - fl(zi^2)) + cr), fl(fl(fl(2 zr) zi) + ci))            the reference's own recurrence
    n = first k with mag_k = fl(fl(zr^2) + fl(zi^2)) >= 4 (k = 1 .. mrd - 1), else 0
    n > 0: run on until mag >= 2^32 or 64 further steps
    de = fl(fl(sqrt(fl(mag / dmag))) fl(ln mag)), 0 if n = 0, 0 instead of NaN

numpy rounds every operation on its own, so the states (n, z, d, mag, dmag) are the contract's bit for bit; only ln can
separate two implementations of de.  expression_true() evaluates the output expression with mpmath at 256 bits on the exact
doubles (mag, dmag), so that glibc's and ocml's results can both be held to the correctly rounded value.

The expression bound, in ulp(de) of the truth's nearest double: the host (mbk_distance_value_host: glibc's ln, IEEE division,
square root and product) is allowed D0, measured by tests/test_distance.py the way smooth_truth.A0 was; the device gets
D0 + 1, one more ulp for ocml's ln (ocml and glibc both aim at <= 1 ulp per call -- the reasoning of smooth_truth.py; here
there is one call, and the product passes its error on to de).  The measure only makes sense while q = mag / dmag is a
normal number: below 2^-1022 the quotient has lost bits before the square root sees it, and there the tests ask for the
model's value itself (through the ln candidates, below).
"""
from __future__ import annotations

import math

import mpmath
import numpy as np

PRECISION_BITS = 256
RUN_ON = 64
RADIUS2 = 2.0 ** 32
# Measured by tests/test_distance.py::test_output_expression_against_mpmath (glibc's libm on x86-64) over the exact
# (mag, dmag) pairs of EXPRESSION_CASES, rounded up to two decimals: the test prints the figure, fails if a pair exceeds it,
# and fails if it is more than 0.1 above what it measures.  Measured 1.9409 at n = 1, mag = 287369839752769.94,
# dmag = 9.725943992673352e+16 (the "ring" view).
D0 = 1.95
D_GPU = D0 + 1.0
# Relative error of the model's de (binary64 orbit and derivative) against the same recurrences at 256 bits, on the escaped
# samples of DERIVATIVE_CASES whose count and run-on length agree: worst measured 8.97e-7 (n = 127, |d| ~ 1e21, in the
# 77 x 53 view; orbits of n <= 30 stay below 5e-13) -> 9e-7 (one digit, rounded up) x 4, the factor because d is an orbit-long
# product whose error grows with n (tests/test_distance.py prints the figure per case).
DERIVATIVE_REL = 3.6e-6


def axes(view, window=None):
    """(cr[ncols], ci[nrows]) of a view tuple (start_r, start_i, range_r, range_i, width, height): np.linspace IS the axis
    (tests/test_oracle.py), and a window's coordinates come from the full view's."""
    sr, si, rr, ri, w, h = view
    c0, r0, nc, nr = window if window is not None else (0, 0, w, h)
    return np.linspace(sr, sr + rr, w)[c0:c0 + nc].copy(), np.linspace(si, si + ri, h)[r0:r0 + nr].copy()


def _step(zr, zi, dr, di, cr, ci):
    p0 = zr * dr
    p1 = zi * di
    p2 = zr * di
    p3 = zi * dr
    u = p0 - p1
    v = p2 + p3
    a = zr * zr
    b = zi * zi
    t = a - b
    w = 2.0 * zr
    q = w * zi
    return t + cr, q + ci, (2.0 * u) + 1.0, 2.0 * v


def _mag(x, y):
    a = x * x
    b = y * y
    return a + b


def states(cr, ci, mrd):
    """Flat arrays cr, ci -> dict of flat arrays: n (int32), extra (run-on steps taken), zr, zi, dr, di, mag, dmag at the final
    state (the initial state where n = 0)."""
    cr = np.asarray(cr, np.float64).ravel()
    ci = np.asarray(ci, np.float64).ravel()
    N = cr.size
    out = {"n": np.zeros(N, np.int32), "extra": np.zeros(N, np.int32)}
    fin = {k: np.zeros(N, np.float64) for k in ("zr", "zi", "dr", "di")}
    fin["zr"][:], fin["zi"][:], fin["dr"][:] = cr, ci, 1.0
    idx = np.arange(N)
    zr, zi, dr, di = cr.copy(), ci.copy(), np.ones(N), np.zeros(N)
    c_r, c_i = cr.copy(), ci.copy()
    with np.errstate(all="ignore"):
        for k in range(1, int(mrd)):
            if idx.size == 0:
                break
            zr, zi, dr, di = _step(zr, zi, dr, di, c_r, c_i)
            esc = _mag(zr, zi) >= 4.0
            if esc.any():
                w = idx[esc]
                out["n"][w] = k
                fin["zr"][w], fin["zi"][w], fin["dr"][w], fin["di"][w] = zr[esc], zi[esc], dr[esc], di[esc]
                keep = ~esc
                idx, zr, zi, dr, di, c_r, c_i = idx[keep], zr[keep], zi[keep], dr[keep], di[keep], c_r[keep], c_i[keep]
        # the run-on of the escaped pixels
        idx = np.flatnonzero(out["n"] > 0)
        zr, zi, dr, di = (fin[k][idx] for k in ("zr", "zi", "dr", "di"))
        c_r, c_i = cr[idx], ci[idx]
        for _ in range(RUN_ON):
            go = ~(_mag(zr, zi) >= RADIUS2)
            if not go.any():
                break
            nzr, nzi, ndr, ndi = _step(zr, zi, dr, di, c_r, c_i)
            zr, zi, dr, di = (np.where(go, a, b) for a, b in ((nzr, zr), (nzi, zi), (ndr, dr), (ndi, di)))
            out["extra"][idx[go]] += 1
        fin["zr"][idx], fin["zi"][idx], fin["dr"][idx], fin["di"][idx] = zr, zi, dr, di
        out.update(fin)
        out["mag"] = _mag(fin["zr"], fin["zi"])
        out["dmag"] = _mag(fin["dr"], fin["di"])
    return out


def value(mag, dmag, n, ln=None):
    """The output expression on arrays; ln: the logarithms to use (default numpy's)."""
    mag = np.asarray(mag, np.float64)
    with np.errstate(all="ignore"):
        q = mag / np.asarray(dmag, np.float64)
        r = np.sqrt(q)
        l = np.log(mag) if ln is None else ln
        de = r * l
    de = np.where(np.isnan(de), 0.0, de)
    return np.where(np.asarray(n) > 0, de, 0.0)


def model(view, mrd, window=None):
    """(de, counts, states) of a view tuple, arrays [nrows, ncols] (states flat)."""
    cr, ci = axes(view, window)
    st = states(np.tile(cr, ci.size), np.repeat(ci, cr.size), mrd)
    shape = (ci.size, cr.size)
    return value(st["mag"], st["dmag"], st["n"]).reshape(shape), st["n"].reshape(shape), st


def ln_candidates(st, reach=2):
    """de for ln within `reach` ulps of numpy's on either side: [2 reach + 1, N].  What an implementation whose states are the
    contract's can store when its ln is within reach ulps of numpy's (each of them within 1 ulp of the truth)."""
    with np.errstate(all="ignore"):
        l = np.log(st["mag"])
        outs = []
        for k in range(-reach, reach + 1):
            lk = l.copy()
            for _ in range(abs(k)):
                lk = np.nextafter(lk, np.inf if k > 0 else -np.inf)
            outs.append(value(st["mag"], st["dmag"], st["n"], ln=lk))
    return np.stack(outs)


def assert_states_agree(got, st, what):
    """`got` (flat de of an implementation) is the model's de bit for bit wherever its ln agrees with numpy's, and elsewhere
    is what a neighbouring ln gives: some candidate matches every sample.  Returns the share that matches numpy's ln itself."""
    got = np.asarray(got, np.float64).ravel()
    cand = ln_candidates(st)
    assert not np.isnan(got).any(), what
    hit = (cand == got[None, :]).any(axis=0)
    assert hit.all(), (what, int((~hit).sum()), [(int(i), int(st["n"][i]), float(st["mag"][i]), float(st["dmag"][i]), float(got[i]),
                                                  float(cand[cand.shape[0] // 2, i])) for i in np.flatnonzero(~hit)[:5]])
    return float((cand[cand.shape[0] // 2] == got).mean())


def expression_true(mag, dmag, n):
    """(nearest double, mpf) of sqrt(mag / dmag) ln mag on the exact doubles; the special cases of the header."""
    mag, dmag = float(mag), float(dmag)
    if int(n) <= 0:
        return 0.0, mpmath.mpf(0)
    if math.isnan(mag) or math.isnan(dmag) or (math.isinf(mag) and math.isinf(dmag)):
        return 0.0, mpmath.mpf(0)
    if math.isinf(mag) or dmag == 0.0:
        return math.inf, mpmath.mpf("inf")
    if math.isinf(dmag):
        return 0.0, mpmath.mpf(0)
    with mpmath.workprec(PRECISION_BITS):
        v = mpmath.sqrt(mpmath.mpf(mag) / mpmath.mpf(dmag)) * mpmath.log(mpmath.mpf(mag))
        return float(v), v


def expression_err_ulps(got, mag, dmag, n):
    """Error of `got` against the truth in ulp(nearest double of the truth), per element; pairs whose q = mag / dmag is not a
    normal number (or whose truth is 0 / inf) give 0 when got equals the truth's nearest double exactly and are otherwise left
    to the caller (nan)."""
    got = np.asarray(got, np.float64).ravel()
    mag = np.asarray(mag, np.float64).ravel()
    dmag = np.asarray(dmag, np.float64).ravel()
    n = np.asarray(n).ravel()
    out = np.zeros(got.size)
    with mpmath.workprec(PRECISION_BITS):
        for i in range(got.size):
            near, v = expression_true(mag[i], dmag[i], n[i])
            normal_q = math.isfinite(mag[i]) and math.isfinite(dmag[i]) and dmag[i] > 0 and mag[i] / dmag[i] >= 2.0 ** -1022
            if n[i] <= 0 or not math.isfinite(near) or near == 0.0 or not normal_q:
                out[i] = 0.0 if got[i] == near else math.nan
                continue
            out[i] = float(abs(mpmath.mpf(float(got[i])) - v) / mpmath.mpf(float(np.spacing(abs(near)))))
    return out


def assert_expression_within(got, st, what, D, pick=None):
    """Every picked sample of `got` within D ulp of the truth at the model's exact (mag, dmag); where q is not normal, a
    candidate of the model's own value (assert_states_agree covers those).  Prints and returns the worst figure."""
    got = np.asarray(got, np.float64).ravel()
    pick = np.arange(got.size) if pick is None else np.asarray(pick)
    e = expression_err_ulps(got[pick], st["mag"][pick], st["dmag"][pick], st["n"][pick])
    ok = ~np.isnan(e)
    worst = float(e[ok].max()) if ok.any() else 0.0
    at = int(pick[ok][np.argmax(e[ok])]) if ok.any() else -1
    print(f"{what}: {int(ok.sum())} samples, worst {worst:.3f} ulp(de) at {at}"
          + (f" (n {int(st['n'][at])}, mag {float(st['mag'][at])!r}, dmag {float(st['dmag'][at])!r})" if at >= 0 else ""))
    assert (e[ok] <= D).all(), (what, worst)
    return worst


def hp_sample(cr, ci, n_model, extra_model):
    """The same recurrences at PRECISION_BITS from the same binary64 c, run for the model's count: (agrees, de as a float).
    agrees: the high-precision orbit escapes at the model's n and runs on for the model's number of steps."""
    with mpmath.workprec(PRECISION_BITS):
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
            return False, math.nan
        extra = 0
        while extra < RUN_ON and not (z.real * z.real + z.imag * z.imag >= RADIUS2):
            d = 2 * z * d + 1
            z = z * z + c
            extra += 1
        if extra != extra_model:
            return False, math.nan
        mag = z.real * z.real + z.imag * z.imag
        dmag = d.real * d.real + d.imag * d.imag
        return True, float(mpmath.sqrt(mag / dmag) * mpmath.log(mag))


# -- the colour rule of MBK_RENDER_DISTANCE ---------------------------------------------------------------------------------
def colour_distance(palette, inside, scale, offset, counts, de):
    """`inside` where the count is 0; else t = fl(fl(de * scale) + offset), t = 0 unless t >= 0; t >= n - 1 (+inf): p[n - 1];
    else k = floor(t), f = floor((t - k) * 256), (p[k] (256 - f) + p[k + 1] f + 128) >> 8 per channel.  No wrap."""
    palette = np.asarray(palette, np.uint8).astype(np.int64)
    n = palette.shape[0]
    assert 2 <= n <= 65536 and 0.0 < scale <= 2.0 ** 80 and abs(offset) <= 2.0 ** 20
    counts = np.asarray(counts, np.int32)
    de = np.asarray(de, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = de * np.float64(scale)
        t = t + np.float64(offset)
    t = np.where(t >= 0.0, t, 0.0)
    last = t >= n - 1
    t = np.where(last, 0.0, t)
    k = np.floor(t)
    f = np.floor((t - k) * 256.0).astype(np.int64)[..., None]
    ki = k.astype(np.int64)
    col = (palette[ki] * (256 - f) + palette[ki + 1] * f + 128) >> 8
    col = np.where(last[..., None], palette[n - 1], col)
    return np.where((counts == 0)[..., None], np.asarray(inside, np.int64), col)


def render_distance(palette, inside, scale, offset, s, counts, de):
    import render_model as R
    return R.resolve(colour_distance(palette, inside, scale, offset, counts, de), s)
