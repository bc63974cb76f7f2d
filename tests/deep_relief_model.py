"""The contract of include/mbk.h, "Relief shading for deep views", in numpy, and its truth -- a helper module, not a conftest.
Written from the header's text, not from the C code.

    state   that of "Distance estimates for deep views" (no table) or of "... with bilinear approximation" (the table of
            deep_bla_model.build): the step helpers of deep_distance_model.py and deep_distance_bla_model.py, and the loop
            written again because their states() do not return the final zp nor the escaping step's mag
    normal  relief_model.normal(zp.r, zp.i, Dr, Di, n): e is not used
    nu      deep_model.smooth_from(n, mag of the ESCAPING step)
    rel     deep_distance_model.value of the final state

tests/test_deep_relief.py asserts that n, extra, Dr, Di, e and the final mag of this loop equal those of the two existing models
on every pixel, which holds the restatement to the two contracts it claims to share.  hp_normal() runs d' = 2 z d + 1,
z' = z^2 + c in mpmath from the exact c = C + dc and returns the unit vector of z / d.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

import deep_bla_model as BL
import deep_distance_bla_model as DB
import deep_distance_model as DD
import deep_model as D
import relief_model as RM

# Euclidean distance between the model's normal and the unit vector of z / d from the same recurrences in mpmath at P + 128
# bits from the exact pixel coordinate, on the escaped picks of tests/test_deep_distance.py::CASES whose count and run-on length
# agree: 64 x 64 views, mrd 3000, 100 picks per case, seed 1 (tests/test_deep_relief.py prints the figure per case and the
# share of picks left out).  name -> (plain, bla).  The error is that of the derivative's direction: the same conditioning of
# the orbit-long product that MEASURED_REL of the two distance models shows for its modulus.
# Every escaped pick agreed in (count, run-on) on every case under both rules: none was left out.  The median over a case's
# picks is 3e-16 .. 6e-14 (plain) and 6e-13 .. 3e-12 (bla): the worst picks are the few where d nearly cancels.
MEASURED_NORMAL = {
    "i-1e-30": (4.0e-14, 2.9e-11), "i-1e-200": (7.7e-14, 6.7e-11), "i-1e-280": (5.2e-12, 1.6e-9), "M51-1e-35": (5.4e-9, 8.4e-7),
    "M41-1e-25": (8.1e-11, 4.1e-9), "seahorse-1e-12": (1.9e-8, 3.4e-6),
}
# the worst figure of each rule, one digit rounded up, x 4: the convention of DEEP_DERIVATIVE_REL
DEEP_NORMAL_ERR = 8e-8         # worst measured 1.9e-8 (seahorse) -> 2e-8 x 4
DEEP_BLA_NORMAL_ERR = 1.6e-5   # worst measured 3.4e-6 (seahorse) -> 4e-6 x 4


def states(zr, zi, dcr, dci, mrd, table=()):
    """Orbit table (zr, zi), flat offsets and the table of deep_bla_model.build (empty: the plain rule) -> dict of flat arrays:
    n (int32), extra (run-on steps taken), zpr, zpi, Dr, Di, e, mag at the final state, dmagD, mag_esc (|z|^2 of the escaping
    step, 0 for n = 0) and steps (executed in the count loop; a skip is one)."""
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    M = zr.size - 1
    T = (zr, zi, zr + zr, zi + zi)
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    extra = np.zeros(N, np.int32)
    steps = np.zeros(N, np.int64)
    fin = {k: np.zeros(N, np.float64) for k in ("Dr", "Di", "mag", "dr", "di", "zpr", "zpi")}
    fin["Dr"][:] = 1.0
    fe = np.zeros(N, np.int64)
    fm = np.zeros(N, np.int64)
    L = len(table)
    off = np.concatenate([[0], np.cumsum([lv["rc"].size for lv in table])]).astype(np.int64)
    flat = {k: (np.concatenate([lv[k] for lv in table]) if L else np.zeros(1)) for k in ("Ar", "Ai", "Br", "Bi", "rc")}
    with np.errstate(all="ignore"):
        idx = np.arange(N)
        m = np.ones(N, np.int64)
        i = np.ones(N, np.int64)
        zpr, zpi = zr[1] + cr, zi[1] + ci                   # z_0 = c = fl(Z_1 + dc)
        dr, di = cr.copy(), ci.copy()
        if M == 1:                                          # no Z_2: rebased at once
            dr, di = zpr.copy(), zpi.copy()
            m[:] = 0
        Dr, Di, e = np.ones(N), np.zeros(N), np.zeros(N, np.int64)
        fin["zpr"][:], fin["zpi"][:] = zpr, zpi             # mrd <= 1 runs no step
        live = i < mrd
        idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e = (a[live] for a in (idx, cr, ci, dr, di, m, i, zpr, zpi, Dr, Di, e))
        while idx.size:
            steps[idx] += 1
            # the level rule of deep_bla_model.counts: the highest level whose conditions all hold, each monotone in the level
            k = m - 1
            ad = np.maximum(np.abs(dr), np.abs(di))
            lvl = np.full(idx.size, -1, np.int64)
            cand = m >= 1
            for t in range(L):
                ok = cand & ((k & ((1 << t) - 1)) == 0) & ((k >> t) < table[t]["rc"].size) & (i + (1 << t) <= mrd)
                ok &= ad < flat["rc"][np.where(ok, off[t] + (k >> t), 0)]
                lvl[ok] = t
                cand = ok
                if not ok.any():
                    break
            took = lvl >= 0
            ls = np.where(took, lvl, 0)
            at = np.where(took, off[ls] + (np.maximum(k, 0) >> ls), 0)
            Ar, Ai, Br, Bi = (flat[q][at] for q in ("Ar", "Ai", "Br", "Bi"))
            # the derivative: across the skip, or the plain step from zp
            sDr, sDi, se = DB.skip(Ar, Ai, Br, Bi, Dr, Di, e)
            pDr, pDi, pe = DD._dstep(zpr, zpi, Dr, Di, e, False)
            Dr, Di, e = np.where(took, sDr, pDr), np.where(took, sDi, pDi), np.where(took, se, pe)
            # dz: the map A dz + B dc, or the plain step; zp is the z formed at the new m
            sr = (Ar * dr - Ai * di) + (Br * c_r - Bi * c_i)
            si = (Ar * di + Ai * dr) + (Br * c_i + Bi * c_r)
            qr, qi = DD._zstep(T, dr, di, m, c_r, c_i)[:2]
            ndr = np.where(took, sr, qr)
            ndi = np.where(took, si, qi)
            m = m + np.where(took, 1 << ls, 1)
            i = i + np.where(took, (1 << ls) - 1, 0)
            zpr = zr[m] + ndr
            zpi = zi[m] + ndi
            mg = zpr * zpr + zpi * zpi
            esc = mg >= 4.0
            w = idx[esc]
            n[w] = i[esc]
            for key, a in (("Dr", Dr), ("Di", Di), ("mag", mg), ("dr", ndr), ("di", ndi), ("zpr", zpr), ("zpi", zpi)):
                fin[key][w] = a[esc]
            fe[w], fm[w] = e[esc], m[esc]
            dr, di, m = DD._rebase(M, ndr, ndi, m, zpr, zpi, mg)
            i = i + 1
            keep = ~esc & (i < mrd)
            gone = ~esc & ~keep           # never escaped: the state of the last step (the outputs are 0 whatever it is)
            g = idx[gone]
            fin["Dr"][g], fin["Di"][g], fe[g], fin["zpr"][g], fin["zpi"][g] = Dr[gone], Di[gone], e[gone], zpr[gone], zpi[gone]
            idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e = (a[keep] for a in (idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e))
        mag_esc = fin["mag"].copy()
        # the run-on of the escaped pixels, plain steps only: first the rebase test the count loop stopped before
        idx = np.flatnonzero(n > 0)
        c_r, c_i = cr[idx], ci[idx]
        Dr, Di, e, mg, zpr, zpi = fin["Dr"][idx], fin["Di"][idx], fe[idx], fin["mag"][idx], fin["zpr"][idx], fin["zpi"][idx]
        dr, di, m = DD._rebase(M, fin["dr"][idx], fin["di"][idx], fm[idx], zpr, zpi, mg)
        for _ in range(DD.RUN_ON):
            go = ~(mg >= DD.RADIUS2)
            if not go.any():
                break
            nDr, nDi, ne = DD._dstep(zpr, zpi, Dr, Di, e, False)
            ndr, ndi, nm, nzr, nzi, nmg = DD._zstep(T, dr, di, m, c_r, c_i)
            ndr, ndi, nm = DD._rebase(M, ndr, ndi, nm, nzr, nzi, nmg)
            Dr, Di, e, dr, di, m, zpr, zpi, mg = (np.where(go, a, b) for a, b in (
                (nDr, Dr), (nDi, Di), (ne, e), (ndr, dr), (ndi, di), (nm, m), (nzr, zpr), (nzi, zpi), (nmg, mg)))
            extra[idx[go]] += 1
        fin["Dr"][idx], fin["Di"][idx], fe[idx], fin["mag"][idx], fin["zpr"][idx], fin["zpi"][idx] = Dr, Di, e, mg, zpr, zpi
        out = {"n": n, "extra": extra, "zpr": fin["zpr"], "zpi": fin["zpi"], "Dr": fin["Dr"], "Di": fin["Di"], "e": fe,
               "mag": fin["mag"], "mag_esc": mag_esc, "steps": steps}
        a = out["Dr"] * out["Dr"]
        b = out["Di"] * out["Di"]
        out["dmagD"] = a + b
    return out


def normals(st):
    """[N, 2] from the states."""
    return RM.normal(st["zpr"], st["zpi"], st["Dr"], st["Di"], st["n"])


def nu(st):
    return D.smooth_from(st["n"], st["mag_esc"])


def model(orbit, view, mrd, window=None, bla=False):
    """(normals [nrows, ncols, 2], counts, nu, rel [nrows, ncols], states) of a DeepView on a DeepOrbit.  The table of bla is
    the FULL view's."""
    zr, zi = orbit.table()
    table = BL.build(zr, zi, BL.dcmax(view)) if bla else ()
    dcr, dci = D.offsets(view, window)
    st = states(zr, zi, dcr, dci, mrd, table)
    shape = (window[3], window[2]) if window is not None else (view.height, view.width)
    rel = DD.value(st["mag"], st["dmagD"], st["e"], view.span_r, st["n"])
    return normals(st).reshape(shape + (2,)), st["n"].reshape(shape), nu(st).reshape(shape), rel.reshape(shape), st


def hp_normal(centre, dc_r, dc_i, n_max, bits):
    """d' = 2 z d + 1, z' = z^2 + c at `bits` bits from the exact c = C + dc, as deep_distance_model.hp_sample runs them, for
    at most n_max counted steps: (n, run-on steps, (nx, ny)), the unit vector of z / d -- that of z conj(d) -- after the
    run-on; n = 0 and NaNs where the orbit has not escaped by n_max.  A model pick is compared where its (n, extra) are these."""
    Cr, Ci = D.exact(centre[0]) + Fraction(float(dc_r)), D.exact(centre[1]) + Fraction(float(dc_i))
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
        while extra < DD.RUN_ON and not (z.real * z.real + z.imag * z.imag >= DD.RADIUS2):
            d = 2 * z * d + 1
            z = z * z + c
            extra += 1
        u = z * mpmath.conj(d)
        u = u / abs(u)
        return n, extra, (float(u.real), float(u.imag))
