"""The contract of include/mbk.h ("Count histograms and histogram-equalised colouring") in numpy, written from the header's
text and not from the C code: np.bincount for the histogram, Python integers for the cumulative sums, one np.float64 division
per table entry, and the value and colour rules on top of tests/render_model.py and tests/distance_model.py's no-wrap rule."""
import numpy as np

import render_model as R

MAX_MRD = 1 << 20


def histogram(counts, mrd):
    """hist[c] = the number of counts equal to c, 0 <= c < mrd; counts outside [0, mrd - 1] are skipped."""
    c = np.asarray(counts, np.int64).ravel()
    c = c[(c >= 0) & (c < mrd)]
    return np.bincount(c, minlength=mrd).astype(np.uint64)


def lut(hist):
    """lut[0] = 0; lut[k] = fl((2 cum(k - 1) + h(k - 1)) / (2 E)) for 1 <= k <= mrd + 1; all zeros when E = 0."""
    h = [int(v) for v in np.asarray(hist, np.uint64)]
    mrd = len(h)
    total = sum(h[1:])
    out = np.zeros(mrd + 2, np.float64)
    if total == 0:
        return out
    assert 2 * total < 2 ** 53
    cum = 0   # cum(k - 1) = sum of h[c] for 1 <= c < min(k - 1, mrd)
    for k in range(1, mrd + 2):
        c = k - 1
        hk = h[c] if 1 <= c < mrd else 0
        out[k] = np.float64(2 * cum + hk) / np.float64(2 * total)
        cum += hk
    return out


def lut_fast(hist):
    """The same table with numpy's exact integer cumulative sums (for long tables); equal to lut() bit for bit while the sums
    stay below 2^53."""
    h = np.asarray(hist, np.uint64).astype(np.int64)
    mrd = h.size
    out = np.zeros(mrd + 2, np.float64)
    hk = np.zeros(mrd + 1, np.int64)          # h(0) .. h(mrd): h(0) = h(mrd) = 0
    hk[1:mrd] = h[1:]
    total = int(hk.sum())
    if total == 0:
        return out
    assert 2 * total < 2 ** 53
    cum = np.concatenate([[0], np.cumsum(hk)[:-1]])   # cum(j) for j = 0 .. mrd
    out[1:] = (2 * cum + hk).astype(np.float64) / np.float64(2 * total)
    return out


def value(table, nu):
    """x = nu, or 0 unless 0 <= x; x >= mrd + 1: lut[mrd + 1]; else k = floor(x), f = x - k,
    v = fl(lut[k] + fl(f * fl(lut[k + 1] - lut[k])))."""
    table = np.asarray(table, np.float64)
    mrd = table.size - 2
    x = np.asarray(nu, np.float64)
    x = np.where(x >= 0.0, x, 0.0)
    top = x >= mrd + 1
    xs = np.where(top, 0.0, x)
    k = np.floor(xs)
    f = xs - k
    ki = k.astype(np.int64)
    d = table[ki + 1] - table[ki]
    p = f * d
    v = table[ki] + p
    return np.where(top, table[mrd + 1], v)


def colour_equalized(palette, inside, scale, offset, table, counts, nu):
    """`inside` where the count is 0; else the MBK_RENDER_DISTANCE rule on v = value(table, nu)."""
    import distance_model as D
    palette = np.asarray(palette, np.uint8)
    assert 0.0 < scale <= 2.0 ** 20
    return D.colour_distance(palette, inside, scale, offset, counts, value(table, nu))


def render_equalized(palette, inside, scale, offset, table, s, counts, nu):
    return R.resolve(colour_equalized(palette, inside, scale, offset, table, counts, nu), s)
