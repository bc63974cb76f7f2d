"""The contract of include/mbk.h, "Relief shading for extended-range deep views", in numpy, and its truth -- a helper module,
not a conftest.  Written from the header's text, not from the C code.

    state   that of "Distance estimates for extended-range deep views" (no table) or of "... with bilinear approximation" (the
            table of deep_wide_bla_model.build): the step helpers of deep_wide_distance_model.py (dstep, _zstep, _rebase) and
            deep_wide_distance_bla_model.py (skip), and the loop written again because their states() return neither the final
            zp = (zr, zi) 2^t nor the escaping step's mag
    normal  relief_model.normal(zr, zi, Dr, Di, n) on the four mantissas: neither t nor e is used
    nu      deep_model.smooth_from(n, mag of the ESCAPING step)
    rel     deep_wide_distance_model.value of the final state

tests/test_deep_wide_relief.py asserts that n, extra, Dr, Di, e, the final mag and dmagD of this loop equal those of the two
existing models on every pick, which holds the restatement to the two contracts it claims to share.  hp_normal() runs
d' = 2 z d + 1, z' = z^2 + c in mpmath from the exact c = C + dcm 2^exp2 and returns the unit vector of z / d.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

import deep_model as D
import deep_wide_bla_model as BL
import deep_wide_distance_bla_model as XD
import deep_wide_distance_model as WD
import deep_wide_model as W
import relief_model as RM

EZ = W.EZ

# Euclidean distance between the model's normal and the unit vector of z / d from the same recurrences in mpmath at P + 128
# bits from the exact pixel coordinate, on the escaped picks of tests/test_deep_wide.py::TRUTH_CASES whose count and run-on
# length agree: the first 100 picks of test_deep_wide._sample, the first 40 on the two 2^-3000 cases
# (tests/test_deep_wide_relief.py prints the figure per case and the number of picks left out).  name -> (plain, xbla).  The
# error is that of the derivative's direction: the conditioning of the orbit-long product that MEASURED_REL of the two wide
# distance models shows for its modulus.  Every escaped pick agreed in (count, run-on) on every case under both rules: none
# was left out.
# The medians are 1e-16 .. 3e-16 (plain) and 6e-13 .. 7e-13 (xbla; 1e-400 takes no skip and keeps the plain figure): the
# worst picks are the few where d nearly cancels.  A skip puts its 2^-40 in place of 2^-53 and replaces up to 2^l roundings by
# one, so c = i moves up and the worst case, the Misiurewicz point at 2^-3000, moves slightly down, as MEASURED_REL does.
MEASURED_NORMAL = {
    "i-1100": (2.5e-13, 1.0e-10), "i-3000": (3.8e-15, 5.2e-12), "mis-1100": (7.4e-11, 2.0e-10), "mis-3000": (1.3e-9, 9.5e-10),
    "1e-400": (8.0e-14, 8.0e-14),
}
# the worst figure of each rule, one digit rounded up, x 4, never wider than 1e-4: the rule of WIDE_DERIVATIVE_REL
WIDE_NORMAL_ERR = 8e-9    # worst measured 1.3e-9 (mis-3000) -> 2e-9 x 4
XBLA_NORMAL_ERR = 4e-9    # worst measured 9.5e-10 (mis-3000) -> 1e-9 x 4


def states(xr, xi, xe, dcr, dci, exp2: int, mrd: int, table=()):
    """Wide orbit table, flat mantissa offsets and the table of deep_wide_bla_model.build (empty: the plain rule) -> dict of
    flat arrays: n (int32), extra (run-on steps taken), zpr, zpi, t (the final z = (zpr, zpi) 2^t), Dr, Di, e (int64), mag at
    the final state, mag_esc (|z|^2 of the escaping step, 0 for n = 0), dmagD, steps (executed in the count loop; a skip is
    one), tmin (the smallest exponent t of a z that a step of the count loop formed, a zero's EZ aside) and xmin (the smallest
    exponent of an orbit entry Z_m, m >= 1, that such a z was formed on)."""
    T = (np.asarray(xr, np.float64), np.asarray(xi, np.float64), np.asarray(xe, np.int64))
    M = T[0].size - 1
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    extra = np.zeros(N, np.int32)
    steps = np.zeros(N, np.int64)
    tmin = np.full(N, 1 << 40, np.int64)
    xmin = np.full(N, 1 << 40, np.int64)
    keys = ("Dr", "Di", "e", "mag", "wr", "wi", "q", "m", "zr", "zi", "t", "mg")
    fin = {k: np.zeros(N, np.int64 if k in ("e", "q", "m", "t") else np.float64) for k in keys}
    L = len(table)
    off = np.concatenate([[0], np.cumsum([lv["ke"].size for lv in table])]).astype(np.int64)
    flat = {k: (np.concatenate([lv[k] for lv in table]) if L else np.zeros(1)) for k in ("Ar", "Ai", "ae", "Br", "Bi", "be", "ke")}
    for k in ("ae", "be", "ke"):
        flat[k] = flat[k].astype(np.int64)
    with np.errstate(all="ignore"):
        idx = np.arange(N)
        m = np.ones(N, np.int64)
        i = np.ones(N, np.int64)
        wr, wi, q = W.norm(cr, ci, np.full(N, exp2, np.int64))
        t, zr, zi, mg = W._z(T[0][m], T[1][m], T[2][m], wr, wi, q)     # z_0 = c
        if M == 1:                                                     # no Z_2: rebased at once
            wr, wi, q = W.norm(zr, zi, t)
            m[:] = 0
        Dr, Di, e = W.norm(np.ones(N), np.zeros(N), np.zeros(N, np.int64))
        for k, a in (("Dr", Dr), ("Di", Di), ("e", e), ("zr", zr), ("zi", zi), ("t", t)):       # mrd <= 1 runs no step
            fin[k][:] = a
        c_r, c_i = cr, ci
        live = i < mrd
        idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t, mg, Dr, Di, e = (a[live] for a in (idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t, mg,
                                                                                      Dr, Di, e))
        while idx.size:
            steps[idx] += 1
            # the level rule of deep_wide_bla_model.counts: the highest level whose conditions all hold, each monotone in it
            k = m - 1
            lvl = np.full(idx.size, -1, np.int64)
            cand = (m >= 1) & (q > EZ)
            for lv in range(L):
                ok = cand & ((k & ((1 << lv) - 1)) == 0) & ((k >> lv) < table[lv]["ke"].size) & (i + (1 << lv) <= mrd)
                ok &= q <= flat["ke"][np.where(ok, off[lv] + (k >> lv), 0)]
                lvl[ok] = lv
                cand = ok
                if not ok.any():
                    break
            took = lvl >= 0
            ls = np.where(took, lvl, 0)
            at = np.where(took, off[ls] + (np.maximum(k, 0) >> ls), 0)
            Ar, Ai, ae, Br, Bi, be = (flat[key][at] for key in ("Ar", "Ai", "ae", "Br", "Bi", "be"))
            # the derivative: across the skip, or the plain step on zp
            sDr, sDi, se = XD.skip(Ar, Ai, ae, Br, Bi, be, Dr, Di, e)
            pDr, pDi, pe = WD.dstep(zr, zi, t, Dr, Di, e)
            Dr, Di, e = np.where(took, sDr, pDr), np.where(took, sDi, pDi), np.where(took, se, pe)
            # dz: the apply rule norm(A w 2^(ae + q) + B dcm 2^(be + exp2)), or the plain steps (a) .. (d)
            p1r, p1i = BL._cmul(Ar, Ai, wr, wi)
            p2r, p2i = BL._cmul(Br, Bi, c_r, c_i)
            e1 = ae + q
            e2 = be + exp2
            h = np.maximum(e1, e2)
            sr, si, sq = W.norm(W.sh(p1r, e1 - h) + W.sh(p2r, e2 - h), W.sh(p1i, e1 - h) + W.sh(p2i, e2 - h), h)
            nr, ni, nq = WD._zstep(T, wr, wi, q, m, c_r, c_i, exp2)[:3]
            wr, wi, q = np.where(took, sr, nr), np.where(took, si, ni), np.where(took, sq, nq)
            m = m + np.where(took, 1 << ls, 1)
            i = i + np.where(took, (1 << ls) - 1, 0)
            # (e), (f): zp is the (zv, t) formed at the new m
            t, zr, zi, mg = W._z(T[0][m], T[1][m], T[2][m], wr, wi, q)
            tmin[idx] = np.minimum(tmin[idx], np.where(t > EZ, t, 1 << 40))
            xmin[idx] = np.minimum(xmin[idx], np.where(T[2][m] > EZ, T[2][m], 1 << 40))
            mag = np.ldexp(mg, (2 * np.maximum(t, -600)).astype(np.int32))
            esc = mag >= 4.0
            w = idx[esc]
            n[w] = i[esc]
            for key, a in zip(keys, (Dr, Di, e, mag, wr, wi, q, m, zr, zi, t, mg)):
                fin[key][w] = a[esc]
            # (g)
            wr, wi, q, m = WD._rebase(M, wr, wi, q, m, zr, zi, t, mg)
            i = i + 1
            keep = ~esc & (i < mrd)
            gone = ~esc & ~keep           # never escaped: the state of the last step (the outputs are 0 whatever it is)
            g = idx[gone]
            for key, a in (("Dr", Dr), ("Di", Di), ("e", e), ("zr", zr), ("zi", zi), ("t", t)):
                fin[key][g] = a[gone]
            idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t, mg, Dr, Di, e = (a[keep] for a in (idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t,
                                                                                          mg, Dr, Di, e))
        mag_esc = fin["mag"].copy()
        # the run-on of the escaped pixels, plain steps only: first the rebase test the count loop stopped before
        idx = np.flatnonzero(n > 0)
        c_r, c_i = cr[idx], ci[idx]
        Dr, Di, e, mag, wr, wi, q, m, zr, zi, t, mg = (fin[k][idx] for k in keys)
        wr, wi, q, m = WD._rebase(M, wr, wi, q, m, zr, zi, t, mg)
        for _ in range(WD.RUN_ON):
            go = ~(mag >= WD.RADIUS2)
            if not go.any():
                break
            new = WD.dstep(zr, zi, t, Dr, Di, e)
            nwr, nwi, nq, nm, nzr, nzi, nt, nmg, nmag = WD._zstep(T, wr, wi, q, m, c_r, c_i, exp2)
            nwr, nwi, nq, nm = WD._rebase(M, nwr, nwi, nq, nm, nzr, nzi, nt, nmg)
            Dr, Di, e, wr, wi, q, m, zr, zi, t, mg, mag = (np.where(go, a, b) for a, b in zip(
                new + (nwr, nwi, nq, nm, nzr, nzi, nt, nmg, nmag), (Dr, Di, e, wr, wi, q, m, zr, zi, t, mg, mag)))
            extra[idx[go]] += 1
        for key, a in (("Dr", Dr), ("Di", Di), ("e", e), ("mag", mag), ("zr", zr), ("zi", zi), ("t", t)):
            fin[key][idx] = a
        out = {"n": n, "extra": extra, "zpr": fin["zr"], "zpi": fin["zi"], "t": fin["t"], "Dr": fin["Dr"], "Di": fin["Di"],
               "e": fin["e"], "mag": fin["mag"], "mag_esc": mag_esc, "steps": steps, "tmin": tmin, "xmin": xmin}
        a = out["Dr"] * out["Dr"]
        b = out["Di"] * out["Di"]
        out["dmagD"] = a + b
    return out


def normals(st):
    """[N, 2] from the states."""
    return RM.normal(st["zpr"], st["zpi"], st["Dr"], st["Di"], st["n"])


def nu(st):
    return D.smooth_from(st["n"], st["mag_esc"])


def rel(st, view):
    return WD.value(st["mag"], st["dmagD"], st["e"], view.range_r, view.exp2, st["n"])


def table_of(orbit, view):
    """The table of the FULL view (deep_wide_bla_model.build); [] for an orbit of length 1."""
    return BL.build(*orbit.wide_table(), BL.dcmax(view))


def model(orbit, view, mrd, window=None, xbla=False):
    """(normals [nrows, ncols, 2], counts, nu, rel [nrows, ncols], states) of a WideDeepView on a DeepOrbit.  The table of xbla
    is the FULL view's."""
    table = table_of(orbit, view) if xbla else ()
    dcr, dci = W.offsets(view, window)
    st = states(*orbit.wide_table(), dcr, dci, view.exp2, mrd, table)
    shape = (window[3], window[2]) if window is not None else (view.height, view.width)
    return normals(st).reshape(shape + (2,)), st["n"].reshape(shape), nu(st).reshape(shape), rel(st, view).reshape(shape), st


def hp_normal(centre, dcm_r, dcm_i, exp2, n_max, bits):
    """d' = 2 z d + 1, z' = z^2 + c at `bits` bits from the exact c = C + dcm 2^exp2, as deep_wide_distance_model.hp_sample
    runs them, for at most n_max counted steps: (n, run-on steps, (nx, ny)), the unit vector of z / d -- that of z conj(d) --
    after the run-on; n = 0 and NaNs where the orbit has not escaped by n_max.  A model pick is compared where its (n, extra)
    are these."""
    s = Fraction(1, 1 << -exp2) if exp2 < 0 else Fraction(1 << exp2)
    Cr, Ci = D.exact(centre[0]) + Fraction(float(dcm_r)) * s, D.exact(centre[1]) + Fraction(float(dcm_i)) * s
    with mpmath.workprec(bits):
        c = mpmath.mpc(mpmath.mpf(Cr.numerator) / Cr.denominator, mpmath.mpf(Ci.numerator) / Ci.denominator)
        z, d = c, mpmath.mpc(1)
        n = 0
        for k in range(1, int(n_max) + 1):
            d = 2 * z * d + 1
            z = z * z + c
            if z.real * z.real + z.imag * z.imag >= 4:
                n = k
                break
        if n == 0:
            return 0, 0, (math.nan, math.nan)
        extra = 0
        while extra < WD.RUN_ON and not (z.real * z.real + z.imag * z.imag >= WD.RADIUS2):
            d = 2 * z * d + 1
            z = z * z + c
            extra += 1
        u = z * mpmath.conj(d)
        u = u / abs(u)
        return n, extra, (float(u.real), float(u.imag))
