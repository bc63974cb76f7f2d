"""The contract of include/mbk.h, "Distance estimates for deep views with bilinear approximation", in numpy -- a helper module,
not a conftest.  Written from the header's text, not from the C code.  Everything of deep_bla_model.py (table, level rule, step
index, counts) and of deep_distance_model.py (the plain derivative step, start state, run-on, output rule, truth) stands; added:

    skip    before the dz map of a step that takes a level, on d = D 2^e and the entry's (A, B):
              ea, eb = the frexp exponents of max(|A_r|, |A_i|), max(|B_r|, |B_i|);  As = ldexp(A, -ea), Bs = ldexp(B, -eb)
              P = (fl(fl(As_r Dr) - fl(As_i Di)), fl(fl(As_r Di) + fl(As_i Dr)));  pe = e + ea;  h = max(pe, eb, 0)
              N = fl(ldexp(P, max(pe - h, -1200)) + ldexp(Bs, max(eb - h, -1200)))
              max(|N_r|, |N_i|) >= 2^256: N = fl(N 2^-256), h += 256;  else < 2^-256 and h >= 256: N = N 2^256, h -= 256
              D = N, e = min(h, 2^30)
    zp      the z = fl(Z_m + dz) every step forms, at the new m after a skip
    run-on  the escaping step's rebase test, then PLAIN steps only

numpy rounds every operation on its own, so the states are the contract's bit for bit; only ln can separate two implementations
of rel (deep_distance_model.ln_candidates / assert_states_agree).
"""
from __future__ import annotations

import numpy as np

import deep_bla_model as BL
import deep_distance_model as DD
import deep_model as D

SHIFT_FLOOR = -1200

# Relative error of the model's rel against d' = 2 z d + 1, z' = z^2 + c in mpmath at P + 128 bits from the exact pixel
# coordinate (deep_distance_model.hp_sample), on the escaped picks of tests/test_deep_distance.py::CASES whose count and run-on
# length agree: 64 x 64 views, mrd 3000, 100 picks per case, seed 1 (tests/test_deep_distance_bla.py prints the figure per
# case).  The error is a conditioning effect of the orbit-long product, not n 2^-39: M51 is far above that.  The picks are a
# sample: over all 4096 pixels of the seahorse view the worst pixel is 3.2e-2 off (the plain model there: 6.0e-5), on pixels
# where d nearly cancels; the 99.9 % quantile of |rel - plain rel| / rel over that view is 1.0e-4.
MEASURED_REL = {
    "i-1e-30": 1.1e-10, "i-1e-200": 1.0e-10, "i-1e-280": 2.7e-9, "M51-1e-35": 2.1e-7, "M41-1e-25": 8.7e-10,
    "seahorse-1e-12": 1.1e-5,
}
# worst measured 1.1e-5 (seahorse, where the plain model's 1.1e-8 is ~1e8 roundings of 2^-53: the same conditioning on the
# skips' 2^-40) -> 2e-5 x 4, the convention of DEEP_DERIVATIVE_REL; under the ceiling of 1e-4 that test_deep_distance.py keeps
DEEP_BLA_DERIVATIVE_REL = 8e-5


def skip(Ar, Ai, Br, Bi, Dr, Di, e):
    """The derivative across a skip on arrays (e: int64): the new (Dr, Di, e)."""
    Ar, Ai, Br, Bi, Dr, Di = (np.asarray(a, np.float64) for a in (Ar, Ai, Br, Bi, Dr, Di))
    e = np.asarray(e, np.int64)
    with np.errstate(all="ignore"):
        ea = np.frexp(np.maximum(np.abs(Ar), np.abs(Ai)))[1].astype(np.int64)
        eb = np.frexp(np.maximum(np.abs(Br), np.abs(Bi)))[1].astype(np.int64)
        asr, asi = np.ldexp(Ar, (-ea).astype(np.int32)), np.ldexp(Ai, (-ea).astype(np.int32))
        bsr, bsi = np.ldexp(Br, (-eb).astype(np.int32)), np.ldexp(Bi, (-eb).astype(np.int32))
        p0 = asr * Dr
        p1 = asi * Di
        p2 = asr * Di
        p3 = asi * Dr
        pr = p0 - p1
        pi = p2 + p3
        pe = e + ea
        h = np.maximum(np.maximum(pe, eb), 0)
        sp = np.maximum(pe - h, SHIFT_FLOOR).astype(np.int32)
        sb = np.maximum(eb - h, SHIFT_FLOOR).astype(np.int32)
        nr = np.ldexp(pr, sp) + np.ldexp(bsr, sb)
        ni = np.ldexp(pi, sp) + np.ldexp(bsi, sb)
        top = np.maximum(np.abs(nr), np.abs(ni))
        big = top >= DD.RESCALE_AT
        small = (top < DD.RESCALE_BY) & (h >= DD.RESCALE_EXP)
        nr = np.where(big, nr * DD.RESCALE_BY, np.where(small, nr * DD.RESCALE_AT, nr))
        ni = np.where(big, ni * DD.RESCALE_BY, np.where(small, ni * DD.RESCALE_AT, ni))
        h = np.where(big, h + DD.RESCALE_EXP, np.where(small, h - DD.RESCALE_EXP, h))
    return nr, ni, np.minimum(h, DD.EXP_CAP)


def states(zr, zi, dcr, dci, mrd, table):
    """Orbit table (zr, zi), flat offsets and the table of deep_bla_model.build -> dict of flat arrays: n (int32), extra (run-on
    steps taken), Dr, Di, e, mag at the final state, dmagD, steps (executed in the count loop; a skip is one)."""
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
        zpr, zpi = zr[1] + cr, zi[1] + ci
        dr, di = cr.copy(), ci.copy()
        if M == 1:
            dr, di = zpr.copy(), zpi.copy()
            m[:] = 0
        Dr, Di, e = np.ones(N), np.zeros(N), np.zeros(N, np.int64)
        c_r, c_i = cr, ci
        live = i < mrd
        idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e = (a[live] for a in (idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e))
        while idx.size:
            steps[idx] += 1
            # the level rule of deep_bla_model.counts
            k = m - 1
            ad = np.maximum(np.abs(dr), np.abs(di))
            lvl = np.full(idx.size, -1, np.int64)
            cand = m >= 1
            for t in range(L):
                nt = table[t]["rc"].size
                ok = cand & ((k & ((1 << t) - 1)) == 0) & ((k >> t) < nt) & (i + (1 << t) <= mrd)
                at = np.where(ok, off[t] + (k >> t), 0)
                ok &= ad < flat["rc"][at]
                lvl[ok] = t
                cand = ok
                if not ok.any():
                    break
            took = lvl >= 0
            ls = np.where(took, lvl, 0)
            at = np.where(took, off[ls] + (np.maximum(k, 0) >> ls), 0)
            Ar, Ai, Br, Bi = (flat[q][at] for q in ("Ar", "Ai", "Br", "Bi"))
            # the derivative: across the skip, or the plain step on zp
            sDr, sDi, se = skip(Ar, Ai, Br, Bi, Dr, Di, e)
            pDr, pDi, pe = DD._dstep(zpr, zpi, Dr, Di, e, False)
            Dr, Di, e = np.where(took, sDr, pDr), np.where(took, sDi, pDi), np.where(took, se, pe)
            # dz: the map, or the plain step
            sr = (Ar * dr - Ai * di) + (Br * c_r - Bi * c_i)
            si = (Ar * di + Ai * dr) + (Br * c_i + Bi * c_r)
            ar = T[2][m] + dr
            ai = T[3][m] + di
            qr = (ar * dr - ai * di) + c_r
            qi = (ar * di + ai * dr) + c_i
            ndr = np.where(took, sr, qr)
            ndi = np.where(took, si, qi)
            m = m + np.where(took, 1 << ls, 1)
            i = i + np.where(took, (1 << ls) - 1, 0)
            zpr = zr[m] + ndr
            zpi = zi[m] + ndi
            mg = zpr * zpr + zpi * zpi
            esc = mg >= 4.0
            if esc.any():
                w = idx[esc]
                n[w] = i[esc]
                for key, a in (("Dr", Dr), ("Di", Di), ("mag", mg), ("dr", ndr), ("di", ndi), ("zpr", zpr), ("zpi", zpi)):
                    fin[key][w] = a[esc]
                fe[w], fm[w] = e[esc], m[esc]
            dr, di, m = DD._rebase(M, ndr, ndi, m, zpr, zpi, mg)
            i = i + 1
            keep = ~esc & (i < mrd)
            gone = ~esc & ~keep           # never escaped: keep the state of the last step (the output is 0 whatever it is)
            fin["Dr"][idx[gone]], fin["Di"][idx[gone]], fe[idx[gone]] = Dr[gone], Di[gone], e[gone]
            idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e = (a[keep] for a in (idx, c_r, c_i, dr, di, m, i, zpr, zpi, Dr, Di, e))
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
        fin["Dr"][idx], fin["Di"][idx], fe[idx], fin["mag"][idx] = Dr, Di, e, mg
        out = {"n": n, "extra": extra, "Dr": fin["Dr"], "Di": fin["Di"], "e": fe, "mag": fin["mag"], "steps": steps}
        a = out["Dr"] * out["Dr"]
        b = out["Di"] * out["Di"]
        out["dmagD"] = a + b
    return out


def model(orbit, view, mrd, window=None):
    """(rel, counts, states) of a DeepView on a DeepOrbit, arrays [nrows, ncols] (states flat).  The table is the FULL view's."""
    zr, zi = orbit.table()
    table = BL.build(zr, zi, BL.dcmax(view))
    dcr, dci = D.offsets(view, window)
    st = states(zr, zi, dcr, dci, mrd, table)
    nrows, ncols = (window[3], window[2]) if window is not None else (view.height, view.width)
    rel = DD.value(st["mag"], st["dmagD"], st["e"], view.span_r, st["n"])
    return rel.reshape(nrows, ncols), st["n"].reshape(nrows, ncols), st
