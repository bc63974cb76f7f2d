"""One sample of a view's axis, and the pixels of a window, without the view -- a helper module like the *_model.py files.

The C oracle (mbo_view) and numpy_view allocate whole axes: 32 GB for an axis of 2^32 - 1 samples.  axis_sample() evaluates
np.linspace's definition (numpy/_core/function_base.py, as oracle/mandel_oracle.c mbo_axis restates it) for chosen indices k
alone, in binary64 with every operation rounded on its own -- numpy never contracts a*b+c:

    stop = start + range;  delta = stop - start;  div = n - 1;  step = delta / div
    y_k  = k * step                     (step != 0)
    y_k  = (k / div) * delta            (step == 0: numpy's fallback)
    x_k  = y_k + start                  two roundings: the product, the sum
    x_{n-1} = stop                      the last sample is pinned;  n == 1: x_0 = start

k is uint64 and is converted to binary64 exactly (k < 2^53), so an index at or above 2^31, or one that a 32-bit sum would
wrap, is what it says.  axis_sample_exact() is the same definition in rational arithmetic with the two roundings made
explicit (tests/test_geometry_limits.py holds one to the other); view_window() gives the coordinate grids of a window, and
window_counts() / window_escape() run the reference loop (oracle.numpy_escape's arithmetic) on them.
"""
from fractions import Fraction

import numpy as np

from oracle.oracle import numpy_escape, numpy_quantise


def _axis_facts(start, rng, n):
    start, rng = np.float64(start), np.float64(rng)
    with np.errstate(all="ignore"):
        stop = start + rng
        delta = stop - start
        div = np.float64(n - 1)
        step = delta / div if n > 1 else np.float64(0.0)
    return start, stop, delta, div, step


def axis_sample(start, rng, n, k, pinned=True) -> np.ndarray:
    """Samples k (array-like of uint64, each < n) of np.linspace(start, start + rng, n).  pinned=False: the regular formula for
    every k, the last one too (what a kernel's fast path evaluates where the host found that it gives `stop` anyway)."""
    n = int(n)
    k = np.asarray(k, dtype=np.uint64)
    assert n >= 1 and (k.size == 0 or int(k.max()) < n), (n, k)
    start, stop, delta, div, step = _axis_facts(start, rng, n)
    if n == 1:
        return np.full(k.shape, start, np.float64)
    kf = k.astype(np.float64)           # exact: k < 2^32 < 2^53
    with np.errstate(all="ignore"):
        if step == 0.0:
            y = kf / div
            y = y * delta
        else:
            y = kf * step
        x = y + start
    return np.where(k == np.uint64(n - 1), stop, x) if pinned else x


def _rn(q: Fraction) -> float:
    """The binary64 nearest to q, ties to even: CPython's int / int is correctly rounded."""
    return q.numerator / q.denominator


def axis_sample_exact(start, rng, n, k: int) -> float:
    """axis_sample for one index in exact rational arithmetic: every operation of the definition is computed exactly and then
    rounded once.  Finite, non-overflowing axes only (what validate_view accepts)."""
    n, k = int(n), int(k)
    assert 0 <= k < n
    start, rng = float(start), float(rng)
    stop = _rn(Fraction(start) + Fraction(rng))
    if n == 1:
        return start
    if k == n - 1:
        return stop
    delta = _rn(Fraction(stop) - Fraction(start))
    step = _rn(Fraction(delta) / (n - 1))
    if step == 0.0:
        y = _rn(Fraction(_rn(Fraction(k, n - 1))) * Fraction(delta))
    else:
        y = _rn(Fraction(k) * Fraction(step))
    return _rn(Fraction(y) + Fraction(start))


def place_view(anchor, step, width, height, window):
    """The six numbers of a width x height view of pixel step `step` whose window (col0, row0, ...) has its first pixel at the
    point `anchor` (to within a few ulp of the view's extent: start + k * step' is not exact)."""
    col0, row0 = int(window[0]), int(window[1])
    return (anchor[0] - col0 * step, anchor[1] - row0 * step, step * (width - 1), step * (height - 1), int(width), int(height))


def _view_tuple(view):
    if hasattr(view, "start_r"):
        return (view.start_r, view.start_i, view.range_r, view.range_i, view.width, view.height)
    return tuple(view)


def window_axes(view, window=None):
    """(xr float64[ncols], xi float64[nrows]) of the window (col0, row0, ncols, nrows) of `view` (a View or its six numbers)."""
    sr, si, rr, ri, w, h = _view_tuple(view)
    col0, row0, ncols, nrows = window if window is not None else (0, 0, w, h)
    assert col0 + ncols <= w and row0 + nrows <= h
    xr = axis_sample(sr, rr, w, np.uint64(col0) + np.arange(ncols, dtype=np.uint64))
    xi = axis_sample(si, ri, h, np.uint64(row0) + np.arange(nrows, dtype=np.uint64))
    return xr, xi


def view_window(view, window=None):
    """(cr, ci), each float64[nrows, ncols]: the coordinates of the window's pixels."""
    xr, xi = window_axes(view, window)
    cr, ci = np.broadcast_arrays(xr[None, :], xi[:, None])
    return np.ascontiguousarray(cr), np.ascontiguousarray(ci)


def window_counts(view, window, mrd, precision="f64"):
    """(counts int32[nrows, ncols], bytes uint8[nrows, ncols]) of the window by oracle.numpy_escape / numpy_quantise."""
    cr, ci = view_window(view, window)
    counts = numpy_escape(cr, ci, mrd, dtype=np.float32 if precision == "f32" else np.float64).reshape(cr.shape)
    return counts, (numpy_quantise(counts, mrd) if mrd > 0 else None)


def window_escape(view, window, mrd):
    """(counts int32, mag float64), each [nrows, ncols]: numpy_escape's loop, keeping |z_n|^2 of the escaping step (the double
    that tripped `>= 4`; 0 where the count is 0) -- what tests/smooth_truth.py evaluates the smooth formula on."""
    cr, ci = view_window(view, window)
    shape = cr.shape
    kr, ki = cr.ravel().copy(), ci.ravel().copy()
    out = np.zeros(kr.shape, np.int32)
    mag = np.zeros(kr.shape, np.float64)
    idx = np.arange(kr.size)
    zr, zi = kr.copy(), ki.copy()
    with np.errstate(all="ignore"):
        for n in range(1, mrd):
            if idx.size == 0:
                break
            t = zr * zr - zi * zi
            u = (2.0 * zr) * zi
            zr = t + kr
            zi = u + ki
            m = zr * zr + zi * zi
            esc = m >= 4.0
            if esc.any():
                out[idx[esc]] = n
                mag[idx[esc]] = m[esc]
                keep = ~esc
                idx, zr, zi, kr, ki = idx[keep], zr[keep], zi[keep], kr[keep], ki[keep]
    return out.reshape(shape), mag.reshape(shape)
