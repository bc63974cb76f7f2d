"""The contract of include/mbk.h, "Deep-zoom views with bilinear approximation", restated for the tests -- a helper module,
not a conftest.  Everything of tests/deep_model.py stands (orbit table, offsets, the plain step, the rebase rule); added:

* dcmax(): the one number a view contributes to the table, fl(|dc_r(column 0)| + |dc_i(row 0)|) of the FULL view;
* build(): the table of (A, B, r, rc) per level, merged pairwise over the orbit, every operation a separate float64 numpy
  operation (numpy never contracts);
* counts(): perturbation with rebasing where a run of 2^l steps is replaced by dz -> A dz + B dc whenever the rule allows,
  vectorised over pixels -- the GPU and mbk_deep_bla_count_host must equal it bit for bit.
"""
from __future__ import annotations

import numpy as np

import deep_model as D

EPS = 2.0 ** -40
HALF_SQRT2 = 0.7071067811865476


def dcmax(view) -> np.float64:
    dr = D.axis_offsets(view.width, view.span_r, [0])[0]
    di = D.axis_offsets(view.height, view.span_i, [0])[0]
    return np.float64(abs(dr) + abs(di))


def _norm(r, i):
    return np.sqrt(r * r + i * i)


def build(zr, zi, dcmax, eps: float = EPS):
    """The table as a list of levels, each a dict of float64 arrays Ar, Ai, Br, Bi, r, rc with n_l = (M - 1) >> l entries;
    [] for M <= 1."""
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    M = zr.size - 1
    levels = []
    if M <= 1:
        return levels
    dcmax = np.float64(dcmax)
    with np.errstate(all="ignore"):
        Ar = zr[1:M] + zr[1:M]
        Ai = zi[1:M] + zi[1:M]
        Br = np.ones(M - 1)
        Bi = np.zeros(M - 1)
        r = np.float64(eps) * _norm(Ar, Ai)
        levels.append(dict(Ar=Ar, Ai=Ai, Br=Br, Bi=Bi, r=r, rc=r * np.float64(HALF_SQRT2)))
        while levels[-1]["r"].size >= 2:
            p = levels[-1]
            n = p["r"].size // 2
            x = {k: v[0:2 * n:2] for k, v in p.items()}
            y = {k: v[1:2 * n:2] for k, v in p.items()}
            Ar = y["Ar"] * x["Ar"] - y["Ai"] * x["Ai"]
            Ai = y["Ar"] * x["Ai"] + y["Ai"] * x["Ar"]
            Br = (y["Ar"] * x["Br"] - y["Ai"] * x["Bi"]) + y["Br"]
            Bi = (y["Ar"] * x["Bi"] + y["Ai"] * x["Br"]) + y["Bi"]
            ax = _norm(x["Ar"], x["Ai"])
            bx = _norm(x["Br"], x["Bi"])
            t = (y["r"] - bx * dcmax) / ax
            ok = (ax != 0.0) & np.isfinite(Ar) & np.isfinite(Ai) & np.isfinite(Br) & np.isfinite(Bi) & np.isfinite(t)
            r = np.where(ok, np.minimum(x["r"], np.maximum(np.where(ok, t, 0.0), 0.0)), 0.0)
            levels.append(dict(Ar=Ar, Ai=Ai, Br=Br, Bi=Bi, r=r, rc=r * np.float64(HALF_SQRT2)))
    return levels


def counts(zr, zi, dcr, dci, mrd: int, table):
    """(counts int32, |z|^2 at the escaping step float64, steps executed int64) per pixel; a skip is one executed step."""
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    M = zr.size - 1
    z2r, z2i = zr + zr, zi + zi
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    n = cr.size
    count = np.zeros(n, np.int32)
    mag = np.zeros(n, np.float64)
    steps = np.zeros(n, np.int64)
    L = len(table)
    off = np.concatenate([[0], np.cumsum([lv["rc"].size for lv in table])]).astype(np.int64)
    flat = {k: (np.concatenate([lv[k] for lv in table]) if L else np.zeros(1)) for k in ("Ar", "Ai", "Br", "Bi", "rc")}
    idx = np.arange(n)
    m = np.ones(n, np.int64)
    i = np.ones(n, np.int64)
    dr, di = cr.copy(), ci.copy()
    if M == 1:
        dr, di = zr[1] + cr, zi[1] + ci
        m[:] = 0
    live = i < mrd
    idx, cr, ci, dr, di, m, i = (a[live] for a in (idx, cr, ci, dr, di, m, i))
    with np.errstate(all="ignore"):
        while idx.size:
            steps[idx] += 1
            # the highest level the rule allows, searched upward from level 0 (every condition is monotone in the level)
            k = m - 1
            ad = np.maximum(np.abs(dr), np.abs(di))
            lvl = np.full(idx.size, -1, np.int64)
            cand = m >= 1
            for t in range(L):
                nt = table[t]["rc"].size
                ok = cand & ((k & ((1 << t) - 1)) == 0) & ((k >> t) < nt) & (i + (1 << t) <= mrd)
                e = np.where(ok, off[t] + (k >> t), 0)
                ok &= ad < flat["rc"][e]
                lvl[ok] = t
                cand = ok
                if not ok.any():
                    break
            skip = lvl >= 0
            ls = np.where(skip, lvl, 0)
            e = np.where(skip, off[ls] + (np.maximum(k, 0) >> ls), 0)
            Ar, Ai, Br, Bi = (flat[q][e] for q in ("Ar", "Ai", "Br", "Bi"))
            sr = (Ar * dr - Ai * di) + (Br * cr - Bi * ci)
            si = (Ar * di + Ai * dr) + (Br * ci + Bi * cr)
            ar = z2r[m] + dr
            ai = z2i[m] + di
            pr = (ar * dr - ai * di) + cr
            pi = (ar * di + ai * dr) + ci
            ndr = np.where(skip, sr, pr)
            ndi = np.where(skip, si, pi)
            m = m + np.where(skip, 1 << ls, 1)
            i = i + np.where(skip, (1 << ls) - 1, 0)
            xr = zr[m] + ndr
            xi = zi[m] + ndi
            mg = xr * xr + xi * xi
            esc = mg >= 4.0
            count[idx[esc]] = i[esc]
            mag[idx[esc]] = mg[esc]
            reb = (mg < ndr * ndr + ndi * ndi) | (m == M)
            dr = np.where(reb, xr, ndr)
            di = np.where(reb, xi, ndi)
            m = np.where(reb, 0, m)
            i = i + 1
            keep = ~esc & (i < mrd)
            idx, cr, ci, dr, di, m, i = (a[keep] for a in (idx, cr, ci, dr, di, m, i))
    return count, mag, steps
