"""The views the deep adaptive-supersampling tests share (include/mbk.h, "Adaptive supersampling of deep views") -- a helper
module, not a conftest.  Every case is a DeepView of span_i = span H / W on the orbit of its centre.

The refined shares are those of tests/adaptive_model.py's mask at the middle threshold on the samples tests/deep_model.py
gives on the library's own orbit table (DeepOrbit.table()), at W x H; tests/test_deep_adaptive.py asserts 5 % .. 60 % for each.
"""
import functools

import numpy as np

import adaptive_model as A
import deep_bla_model as B
import deep_model as D
from distributedmandelbrot_amd import DeepOrbit, DeepView, Palette

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")   # tests/test_gpu_deep_bla.py's
PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255))
SLOW_PAL = Palette.cosine(1000, period=1500, inside=(10, 20, 30, 255))

# name: (centre, span, (W, H), mrd, palette, middle threshold)
#   i-30              the centre pixel is c = i exactly: one interior sample; dcmax is the same at every s          share 0.135
#   i-30-two-tables   dcmax at s = 1 differs from that at every other s                                              share 0.157
#   i-200-two-tables  dcmax differs for every s                                                                       share 0.305
#   M58               M = 58: a skip may end on m == M                                                                share 0.200
#   seahorse          counts 8979 .. 11994, 409 distinct: under PAL every pixel is an edge up to threshold 96 and
#                     beyond, hence the palette of period 1500                                                        share 0.246
CASES = {
    "i-30": (("0", "1"), 1e-30, (67, 45), 3000, PAL, 64),
    "i-30-two-tables": (("0", "1"), 1e-30, (59, 45), 3000, PAL, 64),
    "i-200-two-tables": (("0", "1"), 1e-200, (41, 45), 5000, PAL, 64),
    "M58": (("1e-21", "1"), 1e-20, (67, 45), 5000, PAL, 64),
    "seahorse": (SEAHORSE, 1e-20, (67, 45), 30000, SLOW_PAL, 128),
}
TWO_TABLES = ("i-30-two-tables", "i-200-two-tables")


@functools.lru_cache(maxsize=None)
def orbit(centre, mrd, span):
    return DeepOrbit(*centre, mrd, min_span=span)


def case(name):
    """(orbit, view, mrd, palette, middle threshold)"""
    centre, span, (w, h), mrd, pal, mid = CASES[name]
    return orbit(centre, mrd, span), DeepView(span, w, h, span * h / w), mrd, pal, mid


def finer(view, s):
    return DeepView(view.span_r, view.width * s, view.height * s, view.span_i)


@functools.lru_cache(maxsize=None)
def model_samples(name, s, bla=False):
    """(counts, nu) of the case's view at s times the resolution under the plain contract (deep_model) or, with bla, the
    bilinear-approximation contract (deep_bla_model), on the library's orbit table; computed once and left unchanged."""
    orb, view, mrd, _, _ = case(name)
    view = finer(view, s)
    zr, zi = orb.table()
    dr, di = D.offsets(view)
    if bla:
        c, mag, _ = B.counts(zr, zi, dr, di, mrd, B.build(zr, zi, B.dcmax(view)))
    else:
        c, mag = D.model_counts(zr, zi, dr, di, mrd)
    c = c.reshape(view.height, view.width)
    nu = D.smooth_from(c, mag.reshape(c.shape))
    c.setflags(write=False)
    nu.setflags(write=False)
    return c, nu


def model_share(name, thr):
    _, _, _, pal, _ = case(name)
    c, nu = model_samples(name, 1)
    return float(A.refined_mask(A.base_image(pal.entries, pal.inside, pal.scale, pal.offset, c, nu), thr).mean())
