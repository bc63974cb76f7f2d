"""The interior-view contract (include/mbk.h, "Interior views") in numpy, vectorised over pixels: the Brent schedule is the same
for every pixel, so the search advances all of them in step.  Every operation is one numpy binary64 operation, rounded on its
own; division and square root are numpy's correctly rounded ones.  Nothing here calls the library."""
import numpy as np

TOLERANCE = 2.0 ** -40


def axes(v):
    """(cr[width], ci[height]) of a view tuple (start_r, start_i, range_r, range_i, width, height): np.linspace, as every view."""
    sr, si, rr, ri, w, h = v
    return np.linspace(sr, sr + rr, w), np.linspace(si, si + ri, h)


def step(zr, zi, cr, ci, fma=False):
    """The recurrence of mbk_view_launch: zr' = fl(fl(fl(zr zr) - fl(zi zi)) + cr), zi' = fl(fl(fl(2 zr) zi) + ci).
    fma=True is the kernels' rewrite zi' = fma(2, fl(zr zi), ci): 2 p is exact, so fl(fl(2 p) + ci) is the fused result.  The
    two differ only where zr zi is a non-zero subnormal, and a launch takes the literal form on every view where that can show."""
    if fma:
        return (zr * zr - zi * zi) + cr, (2.0 * (zr * zi)) + ci
    return (zr * zr - zi * zi) + cr, ((2.0 * zr) * zi) + ci


def cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def counts(cr, ci, mrd, fma=False):
    """n: the first k in 1 .. mrd - 1 with fl(fl(zr^2) + fl(zi^2)) >= 4, 0 if there is none."""
    cr, ci = np.asarray(cr, np.float64).ravel(), np.asarray(ci, np.float64).ravel()
    n = np.zeros(cr.size, np.int32)
    idx = np.arange(cr.size)
    zr, zi, ar, ai = cr.copy(), ci.copy(), cr.copy(), ci.copy()
    with np.errstate(all="ignore"):
        for k in range(1, mrd):
            if idx.size == 0:
                break
            zr, zi = step(zr, zi, ar, ai, fma)
            out = zr * zr + zi * zi >= 4.0
            if out.any():
                n[idx[out]] = k
                keep = ~out
                idx, zr, zi, ar, ai = idx[keep], zr[keep], zi[keep], ar[keep], ai[keep]
    return n


def cycle(cr, ci, mrd, fma=False):
    """Stage 2 for pixels whose count is 0: (L, rr, ri, at_window) -- L = 0 where no repeat shows; at_window marks the hits
    that fell on a step with since == w."""
    m = cr.size
    L = np.zeros(m, np.int32)
    at_window = np.zeros(m, bool)
    rr_out, ri_out = cr.copy(), ci.copy()
    idx = np.arange(m)
    zr, zi, ar, ai = cr.copy(), ci.copy(), cr.copy(), ci.copy()
    rr, ri = zr.copy(), zi.copy()
    w, since = 1, 0
    for k in range(1, mrd):
        if idx.size == 0:
            break
        zr, zi = step(zr, zi, ar, ai, fma)
        since += 1
        hit = (zr.view(np.uint64) == rr.view(np.uint64)) & (zi.view(np.uint64) == ri.view(np.uint64))
        if hit.any():
            L[idx[hit]] = since
            at_window[idx[hit]] = since == w
            rr_out[idx[hit]], ri_out[idx[hit]] = rr[hit], ri[hit]
            keep = ~hit
            idx, zr, zi, ar, ai, rr, ri = idx[keep], zr[keep], zi[keep], ar[keep], ai[keep], rr[keep], ri[keep]
        if since == w:
            rr, ri = zr.copy(), zi.copy()
            w, since = 2 * w, 0
    return L, rr_out, ri_out, at_window


def period(rr, ri, cr, ci, L, fma=False):
    """Stage 3: the first d in 1 .. L with max(|yr_d - rr|, |yi_d - ri|) <= 2^-40 (pixels with L > 0)."""
    p = np.zeros(rr.size, np.int32)
    idx = np.arange(rr.size)
    yr, yi = rr.copy(), ri.copy()
    d = 0
    while idx.size:
        d += 1
        yr, yi = step(yr, yi, cr[idx], ci[idx], fma)
        ok = np.maximum(np.abs(yr - rr[idx]), np.abs(yi - ri[idx])) <= TOLERANCE
        assert ok[L[idx] == d].all()      # d = L always qualifies
        p[idx[ok]] = d
        keep = ~ok
        idx, yr, yi = idx[keep], yr[keep], yi[keep]
    return p


def distance(rr, ri, cr, ci, p, fma=False):
    """Stages 4 and 5 (pixels with p > 0)."""
    m = rr.size
    zr, zi = rr.copy(), ri.copy()
    Ar, Ai = np.ones(m), np.zeros(m)
    Br, Bi, Er, Ei, Fr, Fi = (np.zeros(m) for _ in range(6))
    with np.errstate(all="ignore"):
        for k in range(int(p.max()) if m else 0):
            on = k < p
            zFr, zFi = cmul(zr, zi, Fr, Fi)
            ABr, ABi = cmul(Ar, Ai, Br, Bi)
            AAr, AAi = cmul(Ar, Ai, Ar, Ai)
            zEr, zEi = cmul(zr, zi, Er, Ei)
            zBr, zBi = cmul(zr, zi, Br, Bi)
            zAr, zAi = cmul(zr, zi, Ar, Ai)
            nzr, nzi = step(zr, zi, cr, ci, fma)
            new = (2.0 * (zFr + ABr), 2.0 * (zFi + ABi), 2.0 * (AAr + zEr), 2.0 * (AAi + zEi), 2.0 * zBr + 1.0, 2.0 * zBi,
                   2.0 * zAr, 2.0 * zAi, nzr, nzi)     # (2u is exact, so fl(fl(2u) + 1) is the contract's fl(2u + 1))
            Fr, Fi, Er, Ei, Br, Bi, Ar, Ai, zr, zi = (np.where(on, a, b) for a, b in
                                                      zip(new, (Fr, Fi, Er, Ei, Br, Bi, Ar, Ai, zr, zi)))
        m2 = Ar * Ar + Ai * Ai
        gr, gi = 1.0 - Ar, -Ai
        hr, hi = cmul(Er, Ei, Br, Bi)
        tr, ti = cmul(hr, hi, gr, -gi)
        gm = gr * gr + gi * gi
        Gr, Gi = Fr + tr / gm, Fi + ti / gm
        den = Gr * Gr + Gi * Gi
        de = (1.0 - m2) / np.sqrt(den)
        de = np.where(np.isnan(de), 0.0, de)
        de = np.where(m2 < 1.0, de, 0.0)
    return de


def interior(cr, ci, mrd, fma=False):
    """The whole contract for the pixels (cr[k], ci[k]): dict of n, period, cycle (L), de, at_window -- flat arrays.
    fma=True: every stage with the fused doubling (step), which is NOT the contract where the two differ."""
    cr, ci = np.asarray(cr, np.float64).ravel(), np.asarray(ci, np.float64).ravel()
    n = counts(cr, ci, mrd, fma)
    out = {"n": n, "period": np.zeros(n.size, np.int32), "cycle": np.zeros(n.size, np.int32), "de": np.zeros(n.size),
           "at_window": np.zeros(n.size, bool)}
    inside = np.flatnonzero(n == 0)
    if mrd < 2 or inside.size == 0:
        return out
    L, rr, ri, at_window = cycle(cr[inside], ci[inside], mrd, fma)
    out["cycle"][inside] = L
    out["at_window"][inside] = at_window
    s = L > 0
    p = period(rr[s], ri[s], cr[inside][s], ci[inside][s], L[s], fma)
    out["period"][inside[s]] = p
    out["de"][inside[s]] = distance(rr[s], ri[s], cr[inside][s], ci[inside][s], p, fma)
    return out


def view(v, mrd, window=None, fma=False):
    """interior() over a view tuple / window (col0, row0, ncols, nrows): dict of [nrows, ncols] arrays."""
    xr, xi = axes(v)
    c0, r0, nc, nr = window or (0, 0, v[4], v[5])
    cr, ci = np.meshgrid(xr[c0:c0 + nc], xi[r0:r0 + nr])
    return {k: a.reshape(nr, nc) for k, a in interior(cr, ci, mrd, fma).items()}


def colours(palette, unknown, outside, scale, n, period, de):
    """The colour of every sample: uint8[..., 4]."""
    palette = np.asarray(palette, np.uint8).reshape(-1, 4)
    base = palette[(np.maximum(period, 1) - 1) % palette.shape[0]].astype(np.int64)
    with np.errstate(all="ignore"):
        t = de * scale
        f = np.where(t >= 1.0, 256, np.floor(np.where(t >= 1.0, 0.0, t) * 256.0)).astype(np.int64)
    col = base.copy()
    col[..., :3] = (base[..., :3] * f[..., None] + 128) >> 8
    col[(period <= 0) & (n == 0)] = np.asarray(unknown, np.int64)
    col[n > 0] = np.asarray(outside, np.int64)
    return col.astype(np.uint8)


def render(palette, unknown, outside, scale, s, n, period, de):
    """colours() resolved s x s to 1: per channel (2 S + s^2) // (2 s^2)."""
    col = colours(palette, unknown, outside, scale, n, period, de).astype(np.int64)
    h, w = n.shape[0] // s, n.shape[1] // s
    total = col.reshape(h, s, w, s, 4).sum(axis=(1, 3))
    return ((2 * total + s * s) // (2 * s * s)).astype(np.uint8)
