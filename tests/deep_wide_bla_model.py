"""The contract of include/mbk.h, "Extended-range deep views with bilinear approximation", restated for the tests -- a
helper module, not a conftest.  Everything of tests/deep_wide_model.py stands (wide table, offsets, sh, norm, the steps
(a) .. (g)); added:

* dcmax(): the one number a view contributes to the table, (f, e) = real(fl(|dcm_r(column 0)| + |dcm_i(row 0)|), exp2) of
  the FULL view;
* build(): the table of (A, e_A, B, e_B, r, e_r, ke) per level, merged pairwise over the wide orbit table, every operation
  a separate float64 numpy operation on mantissas and int64 exponents (numpy never contracts);
* merge(): one merging step on arrays of entries, which build() is made of (the dead-entry rule can be shown on hand-made
  entries);
* counts(): the wide step where a run of 2^l steps is replaced by dz -> A dz + B dc whenever the rule allows, vectorised
  over pixels -- the GPU and mbk_deep_xbla_count_host must equal it bit for bit.
"""
from __future__ import annotations

import numpy as np

import deep_wide_model as W

EZ = W.EZ
EPS_EXP = -40
HALF_SQRT2 = 0.7071067811865476
MAX_EXP = 1 << 20
KEYS = ("Ar", "Ai", "ae", "Br", "Bi", "be", "rf", "re", "ke")


def real(v, e):
    """The wide real v 2^e, v >= 0: (f in [0.5, 1), exponent), or (0, EZ)."""
    v = np.asarray(v, np.float64)
    f, s = np.frexp(v)
    pos = v > 0.0
    return np.where(pos, f, 0.0), np.where(pos, np.asarray(e, np.int64) + s, EZ)


def cabs(fr, fi, e):
    return real(np.sqrt(fr * fr + fi * fi), e)


def dcmax(view):
    dr, di = W.offsets(view, (0, 0, 1, 1))
    f, e = real(np.abs(dr[0]) + np.abs(di[0]), view.exp2)
    return float(f), int(e)


def _ke(rf, re):
    _, s = np.frexp(rf * np.float64(HALF_SQRT2))
    return np.where(rf == 0.0, EZ, re + s - 1).astype(np.int64)


def _exp_ok(e):
    return (e == EZ) | (np.abs(e) <= MAX_EXP)


def _entries(Ar, Ai, ae, Br, Bi, be, rf, re):
    """Entries from what the formulas gave: dead ones (rf == 0) store zeros at EZ."""
    dead = rf == 0.0
    z = lambda a: np.where(dead, 0.0, a)
    x = lambda a: np.where(dead, EZ, a).astype(np.int64)
    lv = dict(Ar=z(Ar), Ai=z(Ai), ae=x(ae), Br=z(Br), Bi=z(Bi), be=x(be), rf=z(rf), re=x(re))
    lv["ke"] = _ke(lv["rf"], lv["re"])
    return lv


def level0(xr, xi, xe, eps_exp: int = EPS_EXP):
    """Level 0 over the wide table's entries 1 .. M - 1."""
    xr, xi, xe = np.asarray(xr, np.float64), np.asarray(xi, np.float64), np.asarray(xe, np.int64)
    M = xr.size - 1
    ar, ai, xe1 = xr[1:M], xi[1:M], xe[1:M]
    ae = np.where(xe1 == EZ, EZ, xe1 + 1)
    f, e = cabs(ar, ai, ae)
    br, bi, be = W.norm(np.ones(M - 1), np.zeros(M - 1), np.zeros(M - 1, np.int64))
    return _entries(ar, ai, ae, br, bi, be, f, np.where(f == 0.0, EZ, e + eps_exp))


def merge(x, y, dcmax):
    """Entry j of the next level from x = entry 2j and y = entry 2j + 1 (dicts of arrays of equal length)."""
    df, de = np.float64(dcmax[0]), np.int64(dcmax[1])
    with np.errstate(all="ignore"):
        Ar, Ai, ae = W.norm(y["Ar"] * x["Ar"] - y["Ai"] * x["Ai"], y["Ar"] * x["Ai"] + y["Ai"] * x["Ar"], y["ae"] + x["ae"])
        qr = y["Ar"] * x["Br"] - y["Ai"] * x["Bi"]
        qi = y["Ar"] * x["Bi"] + y["Ai"] * x["Br"]
        qe = y["ae"] + x["be"]
        h = np.maximum(qe, y["be"])
        Br, Bi, be = W.norm(W.sh(qr, qe - h) + W.sh(y["Br"], y["be"] - h), W.sh(qi, qe - h) + W.sh(y["Bi"], y["be"] - h), h)
        fa, ea = cabs(x["Ar"], x["Ai"], x["ae"])
        fb, eb = cabs(x["Br"], x["Bi"], x["be"])
        u = fb * df
        ue = eb + de
        g = np.maximum(y["re"], ue)
        d = W.sh(y["rf"], y["re"] - g) - W.sh(u, ue - g)
        live = (x["rf"] != 0.0) & (y["rf"] != 0.0) & (fa != 0.0) & (d > 0.0) & _exp_ok(ae) & _exp_ok(be)
        tf, te = real(np.where(live, d, 0.0) / np.where(live, fa, 1.0), g - ea)
        less = np.where(x["re"] != te, x["re"] < te, x["rf"] < tf)       # r = min(r_x, t)
        rf, re = np.where(less, x["rf"], tf), np.where(less, x["re"], te)
        live &= (rf != 0.0) & (re >= -MAX_EXP)
    return _entries(Ar, Ai, ae, Br, Bi, be, np.where(live, rf, 0.0), re)


def build(xr, xi, xe, dcmax, eps_exp: int = EPS_EXP):
    """The table as a list of levels, each a dict of arrays (KEYS) with n_l = (M - 1) >> l entries; [] for M <= 1."""
    M = np.asarray(xr).size - 1
    if M <= 1:
        return []
    levels = [level0(xr, xi, xe, eps_exp)]
    while levels[-1]["ke"].size >= 2:
        p = levels[-1]
        n = p["ke"].size // 2
        levels.append(merge({k: v[0:2 * n:2] for k, v in p.items()}, {k: v[1:2 * n:2] for k, v in p.items()}, dcmax))
    return levels


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def counts(xr, xi, xe, dcr, dci, exp2: int, mrd: int, table):
    """(counts int32, mag float64 at the escaping step, steps executed int64) per pixel; a skip is one executed step."""
    xr = np.asarray(xr, np.float64)
    xi = np.asarray(xi, np.float64)
    xe = np.asarray(xe, np.int64)
    M = xr.size - 1
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    n = cr.size
    count = np.zeros(n, np.int32)
    mag = np.zeros(n, np.float64)
    steps = np.zeros(n, np.int64)
    L = len(table)
    off = np.concatenate([[0], np.cumsum([lv["ke"].size for lv in table])]).astype(np.int64)
    flat = {k: (np.concatenate([lv[k] for lv in table]) if L else np.zeros(1, table[0][k].dtype if L else np.float64))
            for k in ("Ar", "Ai", "ae", "Br", "Bi", "be", "ke")}
    for k in ("ae", "be", "ke"):
        flat[k] = flat[k].astype(np.int64)
    idx = np.arange(n)
    m = np.ones(n, np.int64)
    i = np.ones(n, np.int64)
    wr, wi, q = W.norm(cr, ci, np.full(n, exp2, np.int64))
    if M == 1:
        t, zr, zi, _ = W._z(xr[m], xi[m], xe[m], wr, wi, q)
        wr, wi, q = W.norm(zr, zi, t)
        m[:] = 0
    live = i < mrd
    idx, cr, ci, wr, wi, q, m, i = (a[live] for a in (idx, cr, ci, wr, wi, q, m, i))
    with np.errstate(all="ignore"):
        while idx.size:
            steps[idx] += 1
            # the highest level the rule allows, searched upward from level 0 (every condition is monotone in the level)
            k = m - 1
            lvl = np.full(idx.size, -1, np.int64)
            cand = (m >= 1) & (q > EZ)
            for t in range(L):
                nt = table[t]["ke"].size
                ok = cand & ((k & ((1 << t) - 1)) == 0) & ((k >> t) < nt) & (i + (1 << t) <= mrd)
                e = np.where(ok, off[t] + (k >> t), 0)
                ok &= q <= flat["ke"][e]
                lvl[ok] = t
                cand = ok
                if not ok.any():
                    break
            skip = lvl >= 0
            ls = np.where(skip, lvl, 0)
            e = np.where(skip, off[ls] + (np.maximum(k, 0) >> ls), 0)
            # the skip
            p1r, p1i = _cmul(flat["Ar"][e], flat["Ai"][e], wr, wi)
            p2r, p2i = _cmul(flat["Br"][e], flat["Bi"][e], cr, ci)
            e1 = flat["ae"][e] + q
            e2 = flat["be"][e] + exp2
            h = np.maximum(e1, e2)
            sr, si, sq = W.norm(W.sh(p1r, e1 - h) + W.sh(p2r, e2 - h), W.sh(p1i, e1 - h) + W.sh(p2i, e2 - h), h)
            # the plain steps a .. d
            x1 = xe[m] + 1
            g = np.maximum(x1, q)
            Ar = W.sh(xr[m], x1 - g) + W.sh(wr, q - g)
            Ai = W.sh(xi[m], x1 - g) + W.sh(wi, q - g)
            pr, pi = _cmul(Ar, Ai, wr, wi)
            pe = g + q
            h = np.maximum(pe, exp2)
            nr, ni, nq = W.norm(W.sh(pr, pe - h) + W.sh(cr, exp2 - h), W.sh(pi, pe - h) + W.sh(ci, exp2 - h), h)
            wr = np.where(skip, sr, nr)
            wi = np.where(skip, si, ni)
            q = np.where(skip, sq, nq)
            m = m + np.where(skip, 1 << ls, 1)
            i = i + np.where(skip, (1 << ls) - 1, 0)
            # e, f, g
            t, zr, zi, mg = W._z(xr[m], xi[m], xe[m], wr, wi, q)
            mgs = np.ldexp(mg, (2 * np.maximum(t, -600)).astype(np.int32))
            esc = mgs >= 4.0
            count[idx[esc]] = i[esc]
            mag[idx[esc]] = mgs[esc]
            dm = wr * wr + wi * wi
            reb = (mg < np.ldexp(dm, (2 * np.maximum(q - t, -600)).astype(np.int32))) | (m == M)
            zr_, zi_, zq = W.norm(zr, zi, t)
            wr = np.where(reb, zr_, wr)
            wi = np.where(reb, zi_, wi)
            q = np.where(reb, zq, q)
            m = np.where(reb, 0, m)
            i = i + 1
            keep = ~esc & (i < mrd)
            idx, cr, ci, wr, wi, q, m, i = (a[keep] for a in (idx, cr, ci, wr, wi, q, m, i))
    return count, mag, steps
