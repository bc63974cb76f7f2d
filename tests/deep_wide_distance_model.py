"""The contract of include/mbk.h, "Distance estimates for extended-range deep views", in numpy, and its truth -- a helper
module, not a conftest.  Written from the header's text, not from the C code.

    state   zp = (zv, t): step (e) on the entry 1 and norm(dcm, exp2) (z_0 = c);  D = norm((1, 0), 0) = (0.5, 0, 1), d = D 2^e
    step    P = (fl(fl(zv_r D_r) - fl(zv_i D_i)), fl(fl(zv_r D_i) + fl(zv_i D_r))), pe = t + e + 1, h = max(pe, 0)
            N = (fl(sh(P_r, pe - h) + sh(1, -h)), sh(P_i, pe - h));  (D, e) = norm(N, h), e = min(e, 2^30)
            then steps (a) .. (g) of deep_wide_model, unchanged; zp = the (zv, t) of step (e)
    n       the wide count; n > 0: (g) on the escaping step's state, then run on until mag >= 2^32 or 64 further steps
    rel     ldexp(fl(fl(fl(sqrt(fl(mag / dmagD))) fl(ln mag)) / f), -(e + k + exp2)),  range_r = f 2^k, 0.5 <= f < 1;
            0 if n = 0, 0 instead of NaN

numpy rounds every operation on its own, so the states (n, extra, D, e, mag, dmagD) are the contract's bit for bit; only ln
can separate two implementations of rel (ln_candidates / assert_states_agree, as in deep_distance_model.py).  hp_sample()
runs d' = 2 z d + 1, z' = z^2 + c in mpmath from the exact c = C + dcm 2^exp2.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

import deep_model as D
import deep_wide_model as W

RUN_ON = 64
RADIUS2 = 2.0 ** 32
EXP_CAP = 1 << 30

# Relative error of the model's rel (binary64 mantissas, the wide perturbed orbit and the wide derivative) against the same
# recurrences in mpmath at P + 128 bits from the exact pixel coordinate, on the escaped picks of
# tests/test_deep_wide.py::TRUTH_CASES whose count and run-on length agree (the first 100 picks of test_deep_wide._sample;
# tests/test_deep_wide_distance.py prints the figure per case, over the first 40 picks on the two 2^-3000 cases: 4.8e-15 and
# 2.0e-9 there).  The constant: the worst measured, one digit rounded up, x 4 because d is an orbit-long product whose error
# grows with n.
MEASURED_REL = {"i-1100": 8.8e-13, "i-3000": 8.8e-13, "mis-1100": 3.9e-11, "mis-3000": 2.0e-9, "1e-400": 7.0e-13}
WIDE_DERIVATIVE_REL = 8e-9    # worst measured 2.0e-9 (mis-3000) -> 2e-9 x 4


def dstep(zr, zi, t, Dr, Di, e):
    """One derivative step on arrays: zp = (zr, zi) 2^t, d = (Dr, Di) 2^e (exponents int64) -> the new (Dr, Di, e)."""
    p0 = zr * Dr
    p1 = zi * Di
    p2 = zr * Di
    p3 = zi * Dr
    Pr = p0 - p1
    Pi = p2 + p3
    pe = t + e + 1
    h = np.maximum(pe, 0)
    Nr = W.sh(Pr, pe - h) + W.sh(np.ones_like(Pr), -h)
    Ni = W.sh(Pi, pe - h)
    Dr, Di, e = W.norm(Nr, Ni, h)
    return Dr, Di, np.minimum(e, EXP_CAP)


def _zstep(T, wr, wi, q, m, cr, ci, exp2):
    """steps (a) .. (e): the new (w, q, m) and (zv, t, mg, mag)"""
    xr, xi, xe = T
    x1 = xe[m] + 1
    g = np.maximum(x1, q)
    Ar = W.sh(xr[m], x1 - g) + W.sh(wr, q - g)
    Ai = W.sh(xi[m], x1 - g) + W.sh(wi, q - g)
    pr = Ar * wr - Ai * wi
    pi = Ar * wi + Ai * wr
    pe = g + q
    h = np.maximum(pe, exp2)
    Nr = W.sh(pr, pe - h) + W.sh(cr, exp2 - h)
    Ni = W.sh(pi, pe - h) + W.sh(ci, exp2 - h)
    wr, wi, q = W.norm(Nr, Ni, h)
    m = m + 1
    t, zr, zi, mg = W._z(xr[m], xi[m], xe[m], wr, wi, q)
    mag = np.ldexp(mg, (2 * np.maximum(t, -600)).astype(np.int32))
    return wr, wi, q, m, zr, zi, t, mg, mag


def _rebase(M, wr, wi, q, m, zr, zi, t, mg):
    """step (g)"""
    dm = wr * wr + wi * wi
    reb = (mg < np.ldexp(dm, (2 * np.maximum(q - t, -600)).astype(np.int32))) | (m == M)
    nr, ni, nq = W.norm(zr, zi, t)
    return np.where(reb, nr, wr), np.where(reb, ni, wi), np.where(reb, nq, q), np.where(reb, 0, m)


def states(xr, xi, xe, dcr, dci, exp2: int, mrd: int):
    """Wide orbit table and flat mantissa offsets -> dict of flat arrays: n (int32), extra (run-on steps taken), Dr, Di, e
    (int64), mag at the final state, dmagD."""
    T = (np.asarray(xr, np.float64), np.asarray(xi, np.float64), np.asarray(xe, np.int64))
    M = T[0].size - 1
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    extra = np.zeros(N, np.int32)
    keys = ("Dr", "Di", "e", "mag", "wr", "wi", "q", "m", "zr", "zi", "t", "mg")
    fin = {k: np.zeros(N, np.int64 if k in ("e", "q", "m", "t") else np.float64) for k in keys}
    with np.errstate(all="ignore"):
        idx = np.arange(N)
        m = np.ones(N, np.int64)
        wr, wi, q = W.norm(cr, ci, np.full(N, exp2, np.int64))
        t, zr, zi, mg = W._z(T[0][m], T[1][m], T[2][m], wr, wi, q)     # z_0 = c
        if M == 1:
            wr, wi, q = W.norm(zr, zi, t)
            m[:] = 0
        Dr, Di, e = W.norm(np.ones(N), np.zeros(N), np.zeros(N, np.int64))
        c_r, c_i = cr, ci
        for i in range(1, int(mrd)):
            if idx.size == 0:
                break
            Dr, Di, e = dstep(zr, zi, t, Dr, Di, e)
            wr, wi, q, m, zr, zi, t, mg, mag = _zstep(T, wr, wi, q, m, c_r, c_i, exp2)
            esc = mag >= 4.0
            if esc.any():
                w = idx[esc]
                n[w] = i
                for k, a in zip(keys, (Dr, Di, e, mag, wr, wi, q, m, zr, zi, t, mg)):
                    fin[k][w] = a[esc]
                keep = ~esc
                idx, c_r, c_i, Dr, Di, e, wr, wi, q, m, zr, zi, t, mg = (a[keep] for a in (idx, c_r, c_i, Dr, Di, e, wr, wi, q, m,
                                                                                          zr, zi, t, mg))
            wr, wi, q, m = _rebase(M, wr, wi, q, m, zr, zi, t, mg)
        # pixels that never escaped keep the derivative of their last step (their output is 0 whatever it is)
        fin["Dr"][idx], fin["Di"][idx], fin["e"][idx] = Dr, Di, e
        # the run-on of the escaped pixels: first the rebase test the count loop stopped before
        idx = np.flatnonzero(n > 0)
        c_r, c_i = cr[idx], ci[idx]
        Dr, Di, e, mag, wr, wi, q, m, zr, zi, t, mg = (fin[k][idx] for k in keys)
        wr, wi, q, m = _rebase(M, wr, wi, q, m, zr, zi, t, mg)
        for _ in range(RUN_ON):
            go = ~(mag >= RADIUS2)
            if not go.any():
                break
            new = dstep(zr, zi, t, Dr, Di, e)
            nwr, nwi, nq, nm, nzr, nzi, nt, nmg, nmag = _zstep(T, wr, wi, q, m, c_r, c_i, exp2)
            nwr, nwi, nq, nm = _rebase(M, nwr, nwi, nq, nm, nzr, nzi, nt, nmg)
            Dr, Di, e, wr, wi, q, m, zr, zi, t, mg, mag = (np.where(go, a, b) for a, b in zip(
                new + (nwr, nwi, nq, nm, nzr, nzi, nt, nmg, nmag), (Dr, Di, e, wr, wi, q, m, zr, zi, t, mg, mag)))
            extra[idx[go]] += 1
        fin["Dr"][idx], fin["Di"][idx], fin["e"][idx], fin["mag"][idx] = Dr, Di, e, mag
        out = {"n": n, "extra": extra, "Dr": fin["Dr"], "Di": fin["Di"], "e": fin["e"], "mag": fin["mag"]}
        a = out["Dr"] * out["Dr"]
        b = out["Di"] * out["Di"]
        out["dmagD"] = a + b
    return out


def value(mag, dmagD, e, range_r, exp2, n, ln=None):
    """The output expression on arrays; ln: the logarithms to use (default numpy's)."""
    mag = np.asarray(mag, np.float64)
    f, k = math.frexp(float(range_r))
    with np.errstate(all="ignore"):
        q = mag / np.asarray(dmagD, np.float64)
        r = np.sqrt(q)
        l = np.log(mag) if ln is None else ln
        de = r * l
        g = de / np.float64(f)
        s = np.clip(-(np.asarray(e, np.int64) + k + int(exp2)), -(1 << 30) - (1 << 15), (1 << 30))   # (fits int32)
        rel = np.ldexp(g, s.astype(np.int32))
    rel = np.where(np.isnan(rel), 0.0, rel)
    return np.where(np.asarray(n) > 0, rel, 0.0)


def model(orbit, view, mrd, window=None):
    """(rel, counts, states) of a WideDeepView on a DeepOrbit, arrays [nrows, ncols] (states flat)."""
    dcr, dci = W.offsets(view, window)
    st = states(*orbit.wide_table(), dcr, dci, view.exp2, mrd)
    nrows, ncols = (window[3], window[2]) if window is not None else (view.height, view.width)
    rel = value(st["mag"], st["dmagD"], st["e"], view.range_r, view.exp2, st["n"])
    return rel.reshape(nrows, ncols), st["n"].reshape(nrows, ncols), st


def ln_candidates(st, range_r, exp2, reach=2):
    """rel for ln within `reach` ulps of numpy's on either side: [2 reach + 1, N]."""
    with np.errstate(all="ignore"):
        l = np.log(st["mag"])
        outs = []
        for j in range(-reach, reach + 1):
            lj = l.copy()
            for _ in range(abs(j)):
                lj = np.nextafter(lj, np.inf if j > 0 else -np.inf)
            outs.append(value(st["mag"], st["dmagD"], st["e"], range_r, exp2, st["n"], ln=lj))
    return np.stack(outs)


def assert_states_agree(got, st, range_r, exp2, what):
    """`got` (flat rel of an implementation) is the model's rel bit for bit wherever its ln agrees with numpy's, and elsewhere
    what a neighbouring ln gives.  Returns the share that matches numpy's ln itself."""
    got = np.asarray(got, np.float64).ravel()
    cand = ln_candidates(st, range_r, exp2)
    assert not np.isnan(got).any(), what
    hit = (cand == got[None, :]).any(axis=0)
    mid = cand.shape[0] // 2
    assert hit.all(), (what, int((~hit).sum()), [(int(i), int(st["n"][i]), float(st["mag"][i]), float(st["dmagD"][i]), int(st["e"][i]),
                                                  float(got[i]), float(cand[mid, i])) for i in np.flatnonzero(~hit)[:5]])
    return float((cand[mid] == got).mean())


def hp_sample(centre, dcm_r, dcm_i, range_r, exp2, n_model, extra_model, bits):
    """d' = 2 z d + 1, z' = z^2 + c at `bits` bits from the exact c = C + dcm 2^exp2, for the model's count and run-on length:
    (agrees, rel = de / (range_r 2^exp2) as a float)."""
    s = Fraction(1, 1 << -exp2) if exp2 < 0 else Fraction(1 << exp2)
    Cr, Ci = D.exact(centre[0]) + Fraction(float(dcm_r)) * s, D.exact(centre[1]) + Fraction(float(dcm_i)) * s
    with mpmath.workprec(bits):
        c = mpmath.mpc(mpmath.mpf(Cr.numerator) / Cr.denominator, mpmath.mpf(Ci.numerator) / Ci.denominator)
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
        span = mpmath.ldexp(mpmath.mpf(float(range_r)), int(exp2))
        return True, float(mpmath.sqrt(mag / dmag) * mpmath.log(mag) / span)
