"""The views the tests of adaptive supersampling of extended-range deep views share (include/mbk.h, the section of that
name) -- a helper module, not a conftest.  Every case is a WideDeepView(range, exp2, W, H, range H / W) on the orbit of its
centre.

The refined shares are those of tests/adaptive_model.py's mask at the middle threshold on the samples tests/deep_wide_model.py
gives on the library's own wide table (DeepOrbit.wide_table()), at W x H; tests/test_deep_wide_adaptive.py asserts 5 % .. 60 %
for each and the figure itself.
"""
import functools

import numpy as np

import adaptive_model as A
import deep_model as D
import deep_wide_bla_model as X
import deep_wide_model as W
from distributedmandelbrot_amd import DeepOrbit, Palette, WideDeepView
from test_deep_wide import MIS, TINY

PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255))

# name: (centre, range, exp2, (W, H), mrd, precision_bits (None: the default for the span), middle threshold)
#   i-1100             the centre pixel is c = i exactly: one interior sample; dcmax is the same at every s          share 0.1506
#   i-1100-two-tables  dcmax at s = 1 differs from that at every other s                                             share 0.1538
#   i-3000-two-tables  the same, at the deepest tested span                                                           share 0.1562
#   mis-1100           a whole row (67 samples) interior                                                              share 0.2882
#   short-1100         the orbit escapes, M = 886 < counts up to 908: rebase at m == M, a skip may end on M           share 0.1532
#   1e-400             every Z_m below 1e-308 at each return: the table exists and no pixel may use it                 share 0.2842
CASES = {
    "i-1100": (("0", "1"), 1.0, -1100, (67, 45), 3000, None, 64),
    "i-1100-two-tables": (("0", "1"), 1.0, -1100, (65, 45), 3000, None, 64),
    "i-3000-two-tables": (("0", "1"), 1.0, -3000, (65, 45), 6000, None, 64),
    "mis-1100": (MIS, 1.0, -1100, (67, 45), 4000, None, 128),
    "short-1100": (("1e-333", "1"), 1.0, -1100, (67, 45), 3000, None, 64),
    "1e-400": (TINY, 4.0, 0, (67, 45), 300, 1408, 64),
}
TWO_TABLES = ("i-1100-two-tables", "i-3000-two-tables")
ONE_TABLE = ("i-1100", "mis-1100", "short-1100", "1e-400")


def wide_view(rng, exp2, w, h):
    return WideDeepView(rng, exp2, w, h, rng * h / w)


@functools.lru_cache(maxsize=None)
def orbit(centre, mrd, min_span_exp2, bits=None):
    return DeepOrbit(*centre, mrd, precision_bits=bits) if bits else DeepOrbit(*centre, mrd, min_span_exp2=min_span_exp2)


def case(name):
    """(orbit, view, mrd, palette, middle threshold)"""
    centre, rng, exp2, (w, h), mrd, bits, mid = CASES[name]
    view = wide_view(rng, exp2, w, h)
    return orbit(centre, mrd, view.min_span_exp2, bits), view, mrd, PAL, mid


def finer(view, s):
    return WideDeepView(view.range_r, view.exp2, view.width * s, view.height * s, view.range_i)


@functools.lru_cache(maxsize=None)
def model_samples(name, s, xbla=False):
    """(counts, nu) of the case's view at s times the resolution under the wide contract (deep_wide_model) or, with xbla, the
    wide bilinear-approximation contract (deep_wide_bla_model), on the library's wide table; computed once and left unchanged."""
    orb, view, mrd, _, _ = case(name)
    view = finer(view, s)
    xr, xi, xe = orb.wide_table()
    dr, di = W.offsets(view)
    if xbla:
        c, mag, _ = X.counts(xr, xi, xe, dr, di, view.exp2, mrd, X.build(xr, xi, xe, X.dcmax(view)))
    else:
        c, mag = W.model_counts(xr, xi, xe, dr, di, view.exp2, mrd)
    c = c.reshape(view.height, view.width)
    nu = D.smooth_from(c, mag.reshape(c.shape))
    c.setflags(write=False)
    nu.setflags(write=False)
    return c, nu


def model_share(name, thr, xbla=False):
    _, _, _, pal, _ = case(name)
    c, nu = model_samples(name, 1, xbla)
    return float(A.refined_mask(A.base_image(pal.entries, pal.inside, pal.scale, pal.offset, c, nu), thr).mean())
