"""The contract of include/mbk.h, "Distance estimates for extended-range deep views with bilinear approximation", in numpy -- a
helper module, not a conftest.  Written from the header's text, not from the C code.  Everything of deep_wide_bla_model.py
(table, level rule, step index, apply rule, counts) and of deep_wide_distance_model.py (the plain derivative step, start
state, run-on, output rule, truth) stands; added:

    skip    before the dz map of a step that takes a level, on d = D 2^e and the entry's (A, e_A), (B, e_B):
              P = (fl(fl(A_r D_r) - fl(A_i D_i)), fl(fl(A_r D_i) + fl(A_i D_r))),  pe = e_A + e,  h = max(pe, e_B)
              N = fl(sh(P, pe - h) + sh(B, e_B - h)) per component;  (D, e) = norm(N, h), e = min(e, 2^30)
    zp      the (zv, t) step (e) forms, at the new m after a skip
    run-on  the escaping step's rebase test, then PLAIN steps only

numpy rounds every operation on its own, so the states are the contract's bit for bit; only ln can separate two implementations
of rel (deep_wide_distance_model.ln_candidates / assert_states_agree).
"""
from __future__ import annotations

import numpy as np

import deep_wide_bla_model as BL
import deep_wide_distance_model as WD
import deep_wide_model as W

EZ = W.EZ

# Relative error of the model's rel against d' = 2 z d + 1, z' = z^2 + c in mpmath at P + 128 bits from the exact pixel
# coordinate (deep_wide_distance_model.hp_sample), on the escaped picks of tests/test_deep_wide.py::TRUTH_CASES whose count and
# run-on length agree: the first 100 picks of test_deep_wide._sample, 40 on the two 2^-3000 cases
# (tests/test_deep_wide_distance_bla.py prints the figure per case).  The full-step wide model measures 8.8e-13 .. 2.0e-9 on
# the same picks: a skip adds its 2^-40 in place of 2^-53 but replaces up to 2^l roundings by one, so c = i moves up (to
# 4.5e-10, as the plain BLA distance's 1e-10 .. 2.7e-9 there) and the worst case, the Misiurewicz point at 2^-3000, moves down.
# 1e-400 takes no skip: the full-step figure.  The constant: the worst measured, one digit rounded up, x 4 because d is an
# orbit-long product whose error grows with n; never wider than 1e-4.
MEASURED_REL = {"i-1100": 4.5e-10, "i-3000": 5.5e-12, "mis-1100": 1.8e-10, "mis-3000": 1.1e-9, "1e-400": 7.0e-13}
XBLA_DERIVATIVE_REL = 8e-9    # worst measured 1.1e-9 (mis-3000) -> 2e-9 x 4


def skip(Ar, Ai, ae, Br, Bi, be, Dr, Di, e):
    """The derivative across a skip on arrays (exponents int64): the new (Dr, Di, e)."""
    Ar, Ai, Br, Bi, Dr, Di = (np.asarray(a, np.float64) for a in (Ar, Ai, Br, Bi, Dr, Di))
    ae, be, e = (np.asarray(a, np.int64) for a in (ae, be, e))
    with np.errstate(all="ignore"):
        p0 = Ar * Dr
        p1 = Ai * Di
        p2 = Ar * Di
        p3 = Ai * Dr
        Pr = p0 - p1
        Pi = p2 + p3
        pe = ae + e
        h = np.maximum(pe, be)
        Nr = W.sh(Pr, pe - h) + W.sh(Br, be - h)
        Ni = W.sh(Pi, pe - h) + W.sh(Bi, be - h)
        nr, ni, ne = W.norm(Nr, Ni, h)
    return nr, ni, np.minimum(ne, WD.EXP_CAP)


def states(xr, xi, xe, dcr, dci, exp2: int, mrd: int, table):
    """Wide orbit table, flat mantissa offsets and the table of deep_wide_bla_model.build -> dict of flat arrays: n (int32),
    extra (run-on steps taken), Dr, Di, e (int64), mag at the final state, dmagD, steps (executed in the count loop; a skip is
    one), first_skip (the step index i of the pixel's first skip, 0 if it took none)."""
    T = (np.asarray(xr, np.float64), np.asarray(xi, np.float64), np.asarray(xe, np.int64))
    M = T[0].size - 1
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    extra = np.zeros(N, np.int32)
    steps = np.zeros(N, np.int64)
    first_skip = np.zeros(N, np.int64)
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
        if M == 1:
            wr, wi, q = W.norm(zr, zi, t)
            m[:] = 0
        Dr, Di, e = W.norm(np.ones(N), np.zeros(N), np.zeros(N, np.int64))
        fin["Dr"][:], fin["Di"][:], fin["e"][:] = Dr, Di, e
        c_r, c_i = cr, ci
        live = i < mrd
        idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t, mg, Dr, Di, e = (a[live] for a in (idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t, mg,
                                                                                      Dr, Di, e))
        while idx.size:
            steps[idx] += 1
            # the level rule of deep_wide_bla_model.counts
            k = m - 1
            lvl = np.full(idx.size, -1, np.int64)
            cand = (m >= 1) & (q > EZ)
            for lv in range(L):
                nt = table[lv]["ke"].size
                ok = cand & ((k & ((1 << lv) - 1)) == 0) & ((k >> lv) < nt) & (i + (1 << lv) <= mrd)
                at = np.where(ok, off[lv] + (k >> lv), 0)
                ok &= q <= flat["ke"][at]
                lvl[ok] = lv
                cand = ok
                if not ok.any():
                    break
            took = lvl >= 0
            ls = np.where(took, lvl, 0)
            at = np.where(took, off[ls] + (np.maximum(k, 0) >> ls), 0)
            first = took & (first_skip[idx] == 0)
            first_skip[idx[first]] = i[first]
            Ar, Ai, ae, Br, Bi, be = (flat[key][at] for key in ("Ar", "Ai", "ae", "Br", "Bi", "be"))
            # the derivative: across the skip, or the plain step on zp
            sDr, sDi, se = skip(Ar, Ai, ae, Br, Bi, be, Dr, Di, e)
            pDr, pDi, pe_ = WD.dstep(zr, zi, t, Dr, Di, e)
            Dr, Di, e = np.where(took, sDr, pDr), np.where(took, sDi, pDi), np.where(took, se, pe_)
            # dz: the apply rule, or the plain steps (a) .. (d)
            p1r, p1i = BL._cmul(Ar, Ai, wr, wi)
            p2r, p2i = BL._cmul(Br, Bi, c_r, c_i)
            e1 = ae + q
            e2 = be + exp2
            h = np.maximum(e1, e2)
            sr, si, sq = W.norm(W.sh(p1r, e1 - h) + W.sh(p2r, e2 - h), W.sh(p1i, e1 - h) + W.sh(p2i, e2 - h), h)
            x1 = T[2][m] + 1
            g = np.maximum(x1, q)
            ar = W.sh(T[0][m], x1 - g) + W.sh(wr, q - g)
            ai = W.sh(T[1][m], x1 - g) + W.sh(wi, q - g)
            pr, pi = BL._cmul(ar, ai, wr, wi)
            pe = g + q
            h = np.maximum(pe, exp2)
            nr, ni, nq = W.norm(W.sh(pr, pe - h) + W.sh(c_r, exp2 - h), W.sh(pi, pe - h) + W.sh(c_i, exp2 - h), h)
            wr = np.where(took, sr, nr)
            wi = np.where(took, si, ni)
            q = np.where(took, sq, nq)
            m = m + np.where(took, 1 << ls, 1)
            i = i + np.where(took, (1 << ls) - 1, 0)
            # (e), (f)
            t, zr, zi, mg = W._z(T[0][m], T[1][m], T[2][m], wr, wi, q)
            mag = np.ldexp(mg, (2 * np.maximum(t, -600)).astype(np.int32))
            esc = mag >= 4.0
            if esc.any():
                w = idx[esc]
                n[w] = i[esc]
                for key, a in zip(keys, (Dr, Di, e, mag, wr, wi, q, m, zr, zi, t, mg)):
                    fin[key][w] = a[esc]
            # (g)
            wr, wi, q, m = WD._rebase(M, wr, wi, q, m, zr, zi, t, mg)
            i = i + 1
            keep = ~esc & (i < mrd)
            gone = ~esc & ~keep           # never escaped: keep the state of the last step (the output is 0 whatever it is)
            fin["Dr"][idx[gone]], fin["Di"][idx[gone]], fin["e"][idx[gone]] = Dr[gone], Di[gone], e[gone]
            idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t, mg, Dr, Di, e = (a[keep] for a in (idx, c_r, c_i, wr, wi, q, m, i, zr, zi, t,
                                                                                          mg, Dr, Di, e))
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
        fin["Dr"][idx], fin["Di"][idx], fin["e"][idx], fin["mag"][idx] = Dr, Di, e, mag
        out = {"n": n, "extra": extra, "Dr": fin["Dr"], "Di": fin["Di"], "e": fin["e"], "mag": fin["mag"], "steps": steps,
               "first_skip": first_skip}
        a = out["Dr"] * out["Dr"]
        b = out["Di"] * out["Di"]
        out["dmagD"] = a + b
    return out


def table_of(orbit, view):
    """The table of the FULL view (deep_wide_bla_model.build)."""
    return BL.build(*orbit.wide_table(), BL.dcmax(view))


def model(orbit, view, mrd, window=None, table=None):
    """(rel, counts, states) of a WideDeepView on a DeepOrbit, arrays [nrows, ncols] (states flat).  The table is the FULL view's."""
    if table is None:
        table = table_of(orbit, view)
    dcr, dci = W.offsets(view, window)
    st = states(*orbit.wide_table(), dcr, dci, view.exp2, mrd, table)
    nrows, ncols = (window[3], window[2]) if window is not None else (view.height, view.width)
    rel = WD.value(st["mag"], st["dmagD"], st["e"], view.range_r, view.exp2, st["n"])
    return rel.reshape(nrows, ncols), st["n"].reshape(nrows, ncols), st


ln_candidates = WD.ln_candidates
assert_states_agree = WD.assert_states_agree
hp_sample = WD.hp_sample
