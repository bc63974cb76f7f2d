"""The contract of density views (include/mbk.h, "Density views") restated in numpy: the samples and their counts, the
orbit points a qualifying sample deposits, the cell rule, the additive table, and the colour / resolve rule of a density
render.  Every numpy float64 operation rounds on its own, which is the contract's arithmetic.  Not a test module.
"""
from __future__ import annotations

import numpy as np

MAX_CELLS = 1 << 28
FACTORS = (1, 2, 4, 8)


def axes(view, window=None):
    """The window's coordinates: np.linspace of the FULL view (what mbk_view_launch computes, bit for bit)."""
    col0, row0, ncols, nrows = window if window is not None else (0, 0, view.width, view.height)
    xs = np.linspace(view.start_r, view.start_r + view.range_r, view.width)[col0:col0 + ncols]
    ys = np.linspace(view.start_i, view.start_i + view.range_i, view.height)[row0:row0 + nrows]
    return xs, ys


def step(zr, zi, cr, ci):
    """The reference's recurrence in its literal form: zi' = fl(fl(fl(2 zr) zi) + c_i)."""
    with np.errstate(over="ignore", invalid="ignore"):
        a = zr * zr
        b = zi * zi
        t = a - b
        w = 2.0 * zr
        q = w * zi
        return t + cr, q + ci


def counts(cr, ci, mrd):
    """calc_mb_value for arrays: the first k >= 1 with |z_k|^2 >= 4 (false for NaN), 0 if none within mrd - 1 updates."""
    n = np.zeros(cr.shape, np.int32)
    zr, zi = cr.copy(), ci.copy()
    live = np.ones(cr.shape, bool)
    for k in range(1, max(int(mrd), 1)):
        if not live.any():
            break
        zr, zi = step(zr, zi, cr, ci)
        with np.errstate(over="ignore", invalid="ignore"):
            mag = zr * zr + zi * zi
        hit = live & (mag >= 4.0)
        n[hit] = k
        live &= ~hit
    return n


def cells(target, zr, zi):
    """(inside, cx, cy) of points: tx = fl(fl(zr - start_r) inv_r), inside iff 0 <= tx < W and 0 <= ty < H (false for NaN),
    the cell (floor tx, floor ty).  cx, cy are 0 where the point is outside."""
    W, H = int(target.width), int(target.height)
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv_r = np.float64(W) / np.float64(target.range_r)
        inv_i = np.float64(H) / np.float64(target.range_i)
        dx = zr - np.float64(target.start_r)
        tx = dx * inv_r
        dy = zi - np.float64(target.start_i)
        ty = dy * inv_i
        inside = (tx >= 0.0) & (tx < W) & (ty >= 0.0) & (ty < H)
    cx = np.where(inside, np.floor(np.where(inside, tx, 0.0)), 0.0).astype(np.int64)
    cy = np.where(inside, np.floor(np.where(inside, ty, 0.0)), 0.0).astype(np.int64)
    return inside, cx, cy


def qualify(n, mrd, min_count=1, max_count=0):
    """The samples that deposit: min_count <= n <= max_count, max_count 0 meaning mrd - 1; n = 0 never."""
    assert min_count >= 1
    hi = max_count if max_count else max(int(mrd) - 1, 0)
    return (n >= min_count) & (n <= hi) & (n > 0)


def accumulate(view, target, mrd, min_count=1, max_count=0, window=None, n=None, coords=None):
    """(table uint64[H, W], deposits, dropped, n) of a window.  The table is exact (no wrap at 2^32: the tests' tables are
    far below it).  coords: the window's (xs, ys) where the caller has them without the view's whole axes
    (tests/geometry_model.py window_axes: a view of 2^32 - 1 samples)."""
    xs, ys = coords if coords is not None else axes(view, window)
    cr, ci = np.meshgrid(xs, ys)
    if n is None:
        n = counts(cr, ci, mrd)
    q = qualify(n, mrd, min_count, max_count)
    table = np.zeros((target.height, target.width), np.uint64)
    deposits = dropped = 0
    cr, ci, nq = cr[q], ci[q], n[q]
    zr, zi = cr.copy(), ci.copy()
    for k in range(int(nq.max()) if nq.size else 0):
        act = k < nq
        inside, cx, cy = cells(target, zr[act], zi[act])
        np.add.at(table, (cy[inside], cx[inside]), 1)
        deposits += int(inside.sum())
        dropped += int((~inside).sum())
        zr, zi = step(zr, zi, cr, ci)
    return table, deposits, dropped, n


def colour(palette, scale, offset, mode, table):
    """A cell v -> g(v) = v ("linear") or fl(sqrt(v)) ("sqrt"); t = fl(fl(g scale) + offset), t = 0 unless t >= 0;
    t >= n - 1: p[n - 1]; else k = floor(t), f = floor((t - k) 256), (p[k] (256 - f) + p[k + 1] f + 128) >> 8 per channel."""
    palette = np.asarray(palette, np.uint8).astype(np.int64)
    n = palette.shape[0]
    assert 2 <= n <= 65536 and 0.0 < scale <= 2.0 ** 80 and abs(offset) <= 2.0 ** 20 and mode in ("linear", "sqrt")
    g = np.asarray(table).astype(np.float64)   # exact: v < 2^32
    if mode == "sqrt":
        g = np.sqrt(g)                          # correctly rounded
    with np.errstate(over="ignore", invalid="ignore"):
        t = g * np.float64(scale)
        t = t + np.float64(offset)
    t = np.where(t >= 0.0, t, 0.0)
    last = t >= n - 1
    t = np.where(last, 0.0, t)
    k = np.floor(t)
    f = np.floor((t - k) * 256.0).astype(np.int64)[..., None]
    ki = k.astype(np.int64)
    col = (palette[ki] * (256 - f) + palette[ki + 1] * f + 128) >> 8
    return np.where(last[..., None], palette[n - 1], col)


def render(palette, scale, offset, mode, factor, table):
    """The image of a table: the colours of its cells, box-filtered over factor x factor cells with the renders' resolve rule,
    (2 S + k^2) // (2 k^2) per channel."""
    c = colour(palette, scale, offset, mode, table)
    h, w, _ = c.shape
    k = int(factor)
    assert k in FACTORS and h % k == 0 and w % k == 0
    total = c.reshape(h // k, k, w // k, k, 4).sum(axis=(1, 3))
    return ((2 * total + k * k) // (2 * k * k)).astype(np.uint8)
