"""The rendering contract of include/mbk.h ("Rendering") in numpy: samples in, RGBA8 out.  Written from the header's text,
not from the C code: per-channel integers throughout, Python's exact integer modulo for the palette index."""
import numpy as np

SUPERSAMPLES = (1, 2, 3, 4, 8)


def colour_bytes(palette, byts):
    """MBK_RENDER_BYTES: p[b]."""
    palette = np.asarray(palette, np.uint8)
    assert palette.shape == (256, 4)
    return palette[np.asarray(byts, np.uint8)].astype(np.int64)


def colour_smooth(palette, inside, scale, offset, counts, nu):
    """MBK_RENDER_SMOOTH: `inside` where the count is 0; else t = fl(fl(nu * scale) + offset), t = 0 unless t >= 0,
    k = floor(t), f = floor((t - k) * 256), (p[k mod n] (256 - f) + p[(k + 1) mod n] f + 128) >> 8 per channel."""
    palette = np.asarray(palette, np.uint8).astype(np.int64)
    n = palette.shape[0]
    assert 2 <= n <= 65536 and 0.0 < scale <= 2.0 ** 20 and abs(offset) <= 2.0 ** 20
    counts = np.asarray(counts, np.int32)
    nu = np.asarray(nu, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = nu * np.float64(scale)        # numpy rounds every operation on its own
        t = t + np.float64(offset)
    t = np.where(t >= 0.0, t, 0.0)        # negative, -inf, NaN
    assert (t < 2.0 ** 52).all(), "outside the contract: no launch produces such a nu"
    k = np.floor(t)
    f = np.floor((t - k) * 256.0).astype(np.int64)
    ki = k.astype(np.int64)               # exact: k < 2^52
    i0 = ki % n
    i1 = (ki + 1) % n
    f = f[..., None]
    col = (palette[i0] * (256 - f) + palette[i1] * f + 128) >> 8
    return np.where((counts == 0)[..., None], np.asarray(inside, np.int64), col)


def resolve(colours, s):
    """(H s, W s, 4) sample colours -> (H, W, 4) uint8: (2 S + s^2) // (2 s^2) of the sum S over each pixel's s x s block."""
    hs, ws, _ = colours.shape
    assert s in SUPERSAMPLES and hs % s == 0 and ws % s == 0
    total = colours.reshape(hs // s, s, ws // s, s, 4).sum(axis=(1, 3))
    out = (2 * total + s * s) // (2 * s * s)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def render_bytes(palette, s, byts):
    return resolve(colour_bytes(palette, byts), s)


def render_smooth(palette, inside, scale, offset, s, counts, nu):
    return resolve(colour_smooth(palette, inside, scale, offset, counts, nu), s)
