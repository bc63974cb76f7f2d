"""Locating minibrots from extended-range deep views on the CPU (include/mbk.h, "Locating minibrots in extended-range deep
views"): the host twin of the wide nucleus kernel against the numpy model of the contract (tests/deep_wide_nucleus_model.py) bit
for bit, the same bits as the plain contract where a plain view can name the spans, the model's atom periods against mpmath at
P + 128 bits, pick_wide_nucleus_seed, and locate_wide_nucleus end to end on host-twin arrays, the round trip view -> nucleus ->
view -> nucleus included.

The two cases, 16 x 16 at span 2^-1100 (found with mpmath at 2700 bits before the code was written): c = i holds a minibrot of
period 883 and size 2^-2203.3998 at (-0.111884, -0.224223) of the span from the centre; the Misiurewicz point of
tests/test_deep_wide.py one of period 1474 and size 2^-2202.4148 at (0.477026, ~0).  Every pixel escapes before step 1600.  Both
test the selection rule: the lowest period of any pixel is 873 (1467), those pixels' targets lie outside the view, and the lowest
period with a target in view is the minibrot's.

Measured here: the separation rule excludes 1 (c = i) and 0 (Misiurewicz) of the 256 pixels and no well-separated pixel differs;
locate_wide_nucleus takes 27 + 22 and 31 + 25 rounds at 2368 bits (a round gains the ~51 bits a binary64 Newton step holds), the
round trip 27 + 13 at 2816 bits (its seed is the first nucleus, good to the 1472 bits its orbit reads), and the 2^-2100 view 42
rounds at 4096 bits before the "precision" verdict.  On i-1e-200 named as a WideDeepView the outputs equal the plain contract's
bits, as on the other two plain cases.
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import deep_model as D
import deep_nucleus_model as NM
import deep_wide_model as W
import deep_wide_nucleus_model as WN
from distributedmandelbrot_amd import (DeepOrbit, DeepView, NucleusError, WideDeepView, deep_nucleus_host, locate_wide_nucleus,
                                       pick_wide_nucleus_seed, wide_nucleus_host, wide_nucleus_precision_bits)
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import device as dv
from test_deep_nucleus import CASES as PLAIN_CASES
from test_deep_nucleus import case as plain_case
from test_deep_nucleus import located as plain_located
from test_deep_wide import MIS

# name: (centre, view, mrd, the period of the minibrot the view holds, its offset from the centre as a fraction of the span,
# log2 of its size)
CASES = {
    "i-2^-1100": (("0", "1"), WideDeepView(1.0, -1100, 16), 1600, 883, (-0.111884, -0.224223), -2203.3998),
    "mis-2^-1100": (MIS, WideDeepView(1.0, -1100, 16), 1600, 1474, (0.477026, 0.0), -2202.4148),
}
LOWEST_PERIOD = {"i-2^-1100": 873, "mis-2^-1100": 1467}   # of any pixel: its target is out of view
N = 16
SEPARATION = 2.0 ** -16   # the two smallest |z_n| must differ by more than this share of the smaller
MAX_EXCLUDED = 5
SAME_AS_PLAIN = ["i-1e-20", "mis-1e-100", "i-1e-200"]


def seeds_of(h, view):
    return h["period"].reshape(view.height, view.width), h["delta"].reshape(view.height, view.width, 2)


@functools.lru_cache(maxsize=None)
def case(name):
    """(orbit, view, host twin arrays, model arrays) of a case; shared, never modified."""
    centre, view, mrd = CASES[name][:3]
    orbit = DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)
    return orbit, view, wide_nucleus_host(orbit, view, np.arange(N * N), mrd), WN.model(orbit, view, mrd)


@functools.lru_cache(maxsize=None)
def located(name):
    orbit, view, h, _ = case(name)
    return locate_wide_nucleus(orbit, view, CASES[name][2], seeds=seeds_of(h, view))


@functools.lru_cache(maxsize=None)
def round_trip():
    """(first nucleus, its orbit, the view that frames it, the host twin arrays, the nucleus located from that view)"""
    first = plain_located("i-1e-200")
    mrd = 4 * first.period
    view, orbit = first.view(17, 17), first.orbit(mrd)
    h = wide_nucleus_host(orbit, view, np.arange(17 * 17), mrd)
    return first, orbit, view, h, locate_wide_nucleus(orbit, view, mrd, seeds=seeds_of(h, view))


def as_wide_view(view: DeepView) -> WideDeepView:
    """the WideDeepView that names the spans of a DeepView"""
    range_r, range_i, exp2 = W.as_wide(view.span_r, view.span_i)
    return WideDeepView(range_r, exp2, view.width, view.height, range_i)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(h, st, what):
    for key in st:
        assert h[key].shape == st[key].shape and h[key].dtype == st[key].dtype, (what, key)
        assert np.array_equal(_bits(h[key]), _bits(st[key])), (what, key, int((_bits(h[key]) != _bits(st[key])).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_model_bit_for_bit(name):
    orbit, view, h, st = case(name)
    assert set(h) == {"n", "period", "best_m", "best_e", "z", "t", "D", "e", "delta"} == set(st)
    _same(h, st, name)
    counts, _ = W.model_counts(*orbit.wide_table(), *W.offsets(view), view.exp2, CASES[name][2])
    assert np.array_equal(h["n"], counts) and (h["n"] > 0).all()        # every pixel escapes before step 1600
    assert np.isfinite(h["delta"]).all() and ((h["best_m"] >= 0.5) & (h["best_m"] < 1.0)).all()
    # the selection rule has work to do: the lowest period of any pixel is not the minibrot's
    assert h["period"].min() == LOWEST_PERIOD[name] < CASES[name][3] and (h["period"] == CASES[name][3]).any()


@pytest.mark.parametrize("centre,view,mrds", [
    (("-2", "0"), WideDeepView(1.0, -1000, 19, 13), (1000,)),            # M == 1: the reference escapes at once
    (("0.26", "0"), WideDeepView(0.8, -4, 19, 13), (300,)),              # the orbit runs out: rebases at m == M
    (("0", "1"), WideDeepView(1.0, -1100, 19, 13), (0, 1, 2, 40))])      # no step, one step, mrd below the period
def test_host_twin_equals_the_model_on_the_edges(centre, view, mrds):
    orbit = DeepOrbit(*centre, max(max(mrds), 2), min_span_exp2=view.min_span_exp2)
    if centre[0] == "-2":
        assert orbit.length == 1
    if centre[0] == "0.26":
        assert orbit.escaped and 1 < orbit.length < 100
    for mrd in mrds:
        h, st = wide_nucleus_host(orbit, view, np.arange(19 * 13), mrd), WN.model(orbit, view, mrd)
        _same(h, st, (centre, mrd))
        assert h["period"].max() <= max(mrd, 1)
        if mrd < 2:
            assert (h["period"] == 1).all() and not h["n"].any()
            assert np.array_equal(h["D"], np.tile([0.5, 0.0], (19 * 13, 1))) and (h["e"] == 1).all()
    if centre[0] == "0.26":
        assert (h["n"] == 0).any() and (h["n"] > orbit.length).any() and len(np.unique(h["period"])) > 3


@pytest.mark.parametrize("name", SAME_AS_PLAIN)
def test_same_bits_as_the_plain_contract(name):
    """Where a plain view can name the spans and the plain run meets no subnormal, period, n and delta are the plain contract's
    bits.  None of the three cases is excused: i-1e-200 meets no subnormal either -- every pixel of these views escapes, so the
    smallest |z|^2 a pixel sees stays above 0.007 (|d| 2^666 times an offset of 1e-201 is of the order of 1), and the 1e+200 of
    the derivative lives in the plain contract's integer e."""
    orbit, view, plain, _ = plain_case(name)
    mrd = PLAIN_CASES[name][2]
    wide = as_wide_view(view)
    assert Fraction(wide.range_r) * Fraction(2) ** wide.exp2 == Fraction(view.span_r)
    h = wide_nucleus_host(orbit, wide, np.arange(N * N), mrd)
    for key in ("period", "n", "delta"):
        assert np.array_equal(_bits(h[key]), _bits(plain[key])), (name, key, int((_bits(h[key]) != _bits(plain[key])).sum()))
    # the kept states are the same numbers: they differ by exact powers of two
    for j in range(0, N * N, 37):
        for k in (0, 1):
            assert Fraction(h["z"][j, k]) * Fraction(2) ** int(h["t"][j]) == Fraction(plain["z"][j, k])
            assert Fraction(h["D"][j, k]) * Fraction(2) ** int(h["e"][j]) == Fraction(plain["D"][j, k]) * Fraction(2) ** int(plain["e"][j])


@pytest.mark.parametrize("name", list(CASES))
def test_model_period_is_mpmaths_argmin(name):
    centre, view, mrd = CASES[name][:3]
    orbit, _, _, st = case(name)
    bits = orbit.precision_bits + 128
    dcr, dci = W.offsets(view)
    excluded, wrong = 0, []
    for j in range(N * N):
        arg, first, second = WN.hp_argmin(centre, dcr[j], dci[j], view.exp2, mrd, bits)
        with mpmath.workprec(bits):
            a, b = mpmath.sqrt(first), mpmath.sqrt(second)
            separated = b - a > SEPARATION * a
        if not separated:
            excluded += 1
        elif arg + 1 != st["period"][j]:
            wrong.append((j, arg + 1, int(st["period"][j])))
    print(f"{name}: {excluded} of {N * N} pixels excluded by the separation rule, {len(wrong)} well-separated pixels differ")
    assert excluded <= MAX_EXCLUDED, excluded
    assert not wrong, wrong[:5]


def _count_host(orbit, view, col, row, mrd):
    cv = dv._cxview(view)
    n, mag = C.c_int32(), C.c_double()
    assert L.load().mbk_deep_xview_count_host(orbit._h, C.byref(cv), col, row, mrd, C.byref(n), C.byref(mag)) == L.MBK_OK
    return n.value


@pytest.mark.parametrize("name", list(CASES))
def test_locate_wide_nucleus_end_to_end_on_host_twin_arrays(name):
    centre, view, mrd, period, where, size_log2 = CASES[name]
    orbit, _, h, _ = case(name)
    nuc = located(name)
    P = nuc.precision_bits
    assert nuc.period == period and nuc.inside is True and nuc.seed_pixel is not None
    assert h["period"][nuc.seed_pixel[0] * N + nuc.seed_pixel[1]] == period
    assert P == wide_nucleus_precision_bits(view) == -(-(2 * 1100 + 128) // 64) * 64 == 2368
    print(f"{name}: period {nuc.period}, {nuc.rounds} + {nuc.polish_rounds} rounds at {P} bits, |size| 2^{nuc.size_log2:.4f}, "
          f"seed pixel {nuc.seed_pixel}")
    c0 = (D.exact(centre[0]), D.exact(centre[1]))
    got = (dv._exact_fraction(nuc.center_r), dv._exact_fraction(nuc.center_i))
    root = NM.hp_newton(got[0], got[1], period, P + 128)      # mpmath, on its own, from the result
    with mpmath.workprec(P + 128):
        c = NM.mpc_of(*got)
        tiny = mpmath.ldexp(1, 40 - P)
        assert abs(c - root) <= tiny, float(mpmath.log(abs(c - root), 2))
        for q in range(1, period):
            if period % q == 0:
                assert abs(NM.hp_z(root, q)) > tiny, q
        _, size = NM.hp_step_and_size(root, period)
        assert abs(nuc.size_log2 - float(mpmath.log(abs(size), 2))) < 1e-6
        assert abs(nuc.size_log2 - size_log2) < 1e-4         # (the table holds four decimals)
        off = (c - NM.mpc_of(*c0)) * mpmath.ldexp(1, -view.exp2) / view.range_r
        assert abs(off.real - where[0]) < 1e-6 and abs(off.imag - where[1]) < 1e-6, (float(off.real), float(off.imag))
    # the view it frames: a WideDeepView with the nucleus in the middle
    v = nuc.view(17)
    assert isinstance(v, WideDeepView) and (v.width, v.height) == (17, 17)
    mrd2 = 4 * period
    o = nuc.orbit(mrd2)
    assert o.length == mrd2
    assert _count_host(o, v, 8, 8, mrd2) == 0


def test_round_trip_from_a_located_nucleus():
    """view -> nucleus -> view -> nucleus: from the plain i-1e-200 nucleus (period 534, size 1.01e-401), its own view(17, 17) --
    a WideDeepView 4 sizes wide -- and its own orbit.  The centre pixel has a zero offset and its Z_534 is about 0, so its
    candidate is the smallest there is.  The second nucleus is the first: the same period and size, a centre within 2^(34 - P) of
    the first's, P the first's precision (the first is a root to about 2^-2140, far closer than that)."""
    first, orbit, view, h, nuc = round_trip()
    assert isinstance(view, WideDeepView) and view.exp2 + math.frexp(view.range_r)[1] - 1 < -960 and first.period == 534
    dcr, dci = W.offsets(view)
    mid = 8 * 17 + 8
    assert dcr[mid] == 0.0 and dci[mid] == 0.0
    xr, xi, xe = (a[534] for a in orbit.wide_table())
    # Z_534 is about 0: the orbit reads P bits of the centre, and Z_p = D_p (C - root) with |D_p| about 1 / sqrt(size)
    assert xe == W.EZ or int(xe) + math.log2(max(abs(xr), abs(xi))) < 8 - first.precision_bits - first.size_log2 / 2
    assert h["period"][mid] == 534 and h["n"][mid] == 0
    # what the wide magnitude is for: as binary64 these smallest |z|^2 are 0 and order nothing
    assert (h["best_e"] < -1100).sum() > 17 and h["best_e"][mid] == h["best_e"].min()
    print(f"round trip: period {nuc.period}, {nuc.rounds} + {nuc.polish_rounds} rounds at {nuc.precision_bits} bits, seed pixel "
          f"{nuc.seed_pixel}, |size| 2^{nuc.size_log2:.6f} against 2^{first.size_log2:.6f}")
    assert nuc.period == 534 and nuc.inside is True
    assert nuc.precision_bits == wide_nucleus_precision_bits(view)
    assert abs(nuc.size_log2 - first.size_log2) < 1e-6
    d = [dv._exact_fraction(a) - dv._exact_fraction(b) for a, b in ((nuc.center_r, first.center_r), (nuc.center_i, first.center_i))]
    assert d[0] * d[0] + d[1] * d[1] <= Fraction(4) ** (34 - first.precision_bits)


def test_precision_verdict_at_the_cap():
    """c = i at span 2^-2100: the minibrot there has a size of about 2^-4203, and 4096 bits -- the cap -- cannot place a view in
    it.  The seed is good to about 2^-2100 and each round gains about 51 bits: the default max_rounds of locate_wide_nucleus,
    max(32, ceil(P / 40)) = 103, lets the refinement converge (42 rounds), so the verdict is "precision"; the 32 rounds that
    locate_nucleus allows end in "not converged"."""
    view = WideDeepView(1.0, -2100, 16)
    mrd = 3000
    orbit = DeepOrbit("0", "1", mrd, min_span_exp2=view.min_span_exp2)
    assert wide_nucleus_precision_bits(view) == 4096
    h = wide_nucleus_host(orbit, view, np.arange(N * N), mrd)
    with pytest.raises(NucleusError) as e:
        locate_wide_nucleus(orbit, view, mrd, seeds=seeds_of(h, view))
    assert e.value.reason == "precision", str(e.value)
    with pytest.raises(NucleusError) as e:
        locate_wide_nucleus(orbit, view, mrd, seeds=seeds_of(h, view), max_rounds=32)
    assert e.value.reason == "not converged"


def test_no_seed_and_plain_views_are_refused():
    orbit, view, h, _ = case("i-2^-1100")
    with pytest.raises(NucleusError) as e:
        locate_wide_nucleus(orbit, view, 1600, seeds=(h["period"].reshape(N, N), np.full((N, N, 2), np.inf)))
    assert e.value.reason == "no seed"
    plain = DeepView(1e-20, N, N)
    with pytest.raises(ValueError):
        locate_wide_nucleus(orbit, plain, 1600, seeds=seeds_of(h, view))
    with pytest.raises(ValueError):
        pick_wide_nucleus_seed(plain, *seeds_of(h, view))
    with pytest.raises(ValueError):
        wide_nucleus_host(orbit, plain, [0], 1600)


def test_wide_nucleus_precision_bits():
    assert wide_nucleus_precision_bits(WideDeepView(1.0, -1100, 16)) == 2368
    assert wide_nucleus_precision_bits(WideDeepView(1.0, -1000, 16)) == 2176           # 2128 -> the next multiple of 64
    assert wide_nucleus_precision_bits(WideDeepView(0.75, -1000, 16)) == 2176          # min_span_exp2 -1001: 2130
    assert wide_nucleus_precision_bits(WideDeepView(1.0, -992, 16)) == 2112            # 2112 is a multiple already
    assert wide_nucleus_precision_bits(WideDeepView(4.0, 0, 16)) == 128
    assert wide_nucleus_precision_bits(WideDeepView(1.0, -1984, 16)) == 4096
    assert wide_nucleus_precision_bits(WideDeepView(1.0, -8192, 16)) == 4096
    assert wide_nucleus_precision_bits(WideDeepView(1.0, -1100, 16, 8, range_i=2.0 ** -40)) == 2432    # the smaller span counts: 2 x 1140 + 128


def test_pick_wide_nucleus_seed_on_hand_made_arrays():
    view = WideDeepView(1.0, -1100, 5, 5)                    # pixel offsets -0.5, -0.25, 0, 0.25, 0.5 (x 2^-1100) on both axes
    unit = Fraction(2) ** -1100
    period = np.full((5, 5), 9, np.int32)
    delta = np.zeros((5, 5, 2))
    delta[..., 0] = 0.125
    delta[:, 4, 0] = 0.001                                   # column 4: 0.5 + 0.001 is out of view
    s = pick_wide_nucleus_seed(view, period, delta)
    assert s.pixel == (0, 0) and s.period == 9 and (s.offset_r, s.offset_i) == (Fraction(-3, 8) * unit, Fraction(-1, 2) * unit)
    # the lowest period wins over a smaller |delta| ...
    period[3, 1] = 4
    delta[2, 2] = (0.01, 0.0)
    s = pick_wide_nucleus_seed(view, period, delta)
    assert s.pixel == (3, 1) and s.period == 4 and (s.offset_r, s.offset_i) == (Fraction(-1, 8) * unit, Fraction(1, 4) * unit)
    # ... unless its target is out of view, or its delta is inf
    delta[3, 1] = (0.9, 0.0)
    assert pick_wide_nucleus_seed(view, period, delta).pixel == (2, 2)
    delta[3, 1] = (np.inf, np.inf)
    period[0, 4] = 2
    assert pick_wide_nucleus_seed(view, period, delta).pixel == (2, 2)
    # among equal periods the smallest |delta|, then image order
    delta[2, 2] = (0.125, 0.0)
    delta[1, 3] = (0.0, -0.0625)
    delta[4, 0] = (0.0625, 0.0)
    assert pick_wide_nucleus_seed(view, period, delta).pixel == (1, 3)
    delta[1, 3] = (0.0625, 0.0)                              # now equal to (4, 0)'s: the first in image order
    assert pick_wide_nucleus_seed(view, period, delta).pixel == (1, 3)
    delta[1, 3] = (np.nextafter(0.0625, 1.0), 0.0)           # one ulp more: inside the 1e-12 band, decided exactly
    assert pick_wide_nucleus_seed(view, period, delta).pixel == (4, 0)
    # an underflowed delta (0) is a valid value: the pixel is its own target
    zero = np.full((5, 5, 2), np.inf)
    zero[3, 3] = (0.0, -0.0)
    s = pick_wide_nucleus_seed(view, period, zero)
    assert s.pixel == (3, 3) and (s.offset_r, s.offset_i) == (Fraction(1, 4) * unit, Fraction(1, 4) * unit)
    assert pick_wide_nucleus_seed(view, period, np.full((5, 5, 2), np.inf)) is None
    assert pick_wide_nucleus_seed(view, period, np.full((5, 5, 2), 3.0)) is None
    # the range is a mantissa, not 1: a view 0.75 x 2^-2000 wide
    view = WideDeepView(0.75, -2000, 4, 4)                   # offsets -0.375, -0.125, 0.125, 0.375
    one = np.full((4, 4, 2), np.inf)
    one[1, 2] = (0.25, -0.5)                                 # target (0.125 + 0.25 x 0.75, -0.125 - 0.5 x 0.75) = (0.3125, -0.5): out
    assert pick_wide_nucleus_seed(view, np.ones((4, 4), np.int32), one) is None
    one[1, 2] = (0.25, -0.25)                                # (0.3125, -0.3125): in
    s = pick_wide_nucleus_seed(view, np.ones((4, 4), np.int32), one)
    assert s.pixel == (1, 2) and (s.offset_r, s.offset_i) == (Fraction(5, 16) * Fraction(2) ** -2000, Fraction(-5, 16) * Fraction(2) ** -2000)


def test_pick_wide_nucleus_seed_decides_the_edge_band_exactly():
    """Targets within 1e-12 (relative) of an edge are outside the float pre-test's reach: the exact path decides them."""
    view = WideDeepView(1.0, -1100, 5, 5)
    period = np.full((5, 5), 7, np.int32)
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            edge = np.full((5, 5, 2), np.inf)
            r, c = (2, 3 if sign > 0 else 1) if axis == 0 else (3 if sign > 0 else 1, 2)      # the pixel at +-0.25 on that axis
            inside = np.nextafter(0.25, 0.0)                # target 0.5 - 2.8e-17: in the band, inside
            outside = np.nextafter(0.25, 1.0)               # target 0.5 + 5.6e-17: in the band, outside
            for d, want in ((inside, True), (0.25, True), (outside, False), (0.25 - 1e-13, True), (0.25 + 1e-13, False)):
                edge[r, c] = (0.0, 0.0)
                edge[r, c, axis] = sign * d
                s = pick_wide_nucleus_seed(view, period, edge)
                assert (s is not None) == want, (axis, sign, d)
                if want:
                    assert s.pixel == (r, c)
                    t = (s.offset_r, s.offset_i)[axis] * Fraction(2) ** 1100
                    assert t == Fraction(sign * 0.25) + Fraction(sign * d) and abs(t) * 2 <= 1
    # the float sum rounds both neighbours of the edge onto it: only the exact path can tell them apart
    assert 0.25 + np.nextafter(0.25, 0.0) == 0.5 or 0.25 + np.nextafter(0.25, 1.0) == 0.5


def test_validator_refusals_through_the_host_call():
    lib = L.load()
    orbit = DeepOrbit("0", "1", 500, min_span_exp2=-1101)
    view = WideDeepView(1.0, -1100, 16, 16)
    good = dv._cxview(view)
    n, p, be, t, e, bm = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7), C.c_int32(-7), C.c_int32(-7), C.c_double(-7.0)
    z, d, delta = (C.c_double * 2)(-7.0, -7.0), (C.c_double * 2)(-7.0, -7.0), (C.c_double * 2)(-7.0, -7.0)
    outs = [C.byref(n), C.byref(p), C.byref(bm), C.byref(be), z, C.byref(t), d, C.byref(e), delta]

    def refused(text, o=orbit._h, v=good, col=0, row=0, mrd=100, args=outs):
        rc = lib.mbk_deep_xview_nucleus_host(o, C.byref(v) if v is not None else None, col, row, mrd, *args)
        assert rc == L.MBK_ERR_INVALID, text
        assert text in dv._error_text(lib), (text, dv._error_text(lib))

    for k in range(len(outs)):
        refused("NULL argument", args=outs[:k] + [None] + outs[k + 1:])
    refused("orbit is NULL", o=None)
    refused("view is NULL", v=None)
    refused("mrd exceeds the mrd the reference orbit was computed for", mrd=501)
    refused("pixel outside the view", col=16)
    refused("pixel outside the view", row=16)
    refused("empty view", v=L.mbk_deep_xview(1.0, 1.0, -1100, 0, 16, 0, 0, 0, 16))
    refused("empty window", v=dv._cxview(view, (0, 0, 0, 16)))
    refused("window exceeds the view", v=dv._cxview(view, (10, 0, 7, 16)))
    for rng in (2.0 ** -65, 4.5, float("nan"), float("inf"), -1.0):
        refused("ranges must be finite and lie in [2^-64, 4]", v=dv._cxview(WideDeepView(rng, -1100, 16, 16)))
        refused("ranges must be finite and lie in [2^-64, 4]", v=dv._cxview(WideDeepView(1.0, -1100, 16, 16, range_i=rng)))
    for exp2 in (1, -8193):
        refused("exp2 must lie in [-8192, 0]", v=dv._cxview(WideDeepView(1.0, exp2, 16, 16)))
    assert (n.value, p.value, be.value, t.value, e.value, bm.value) == (-7, -7, -7, -7, -7, -7.0)
    assert tuple(z) == tuple(d) == tuple(delta) == (-7.0, -7.0)
    # and the call itself
    assert lib.mbk_deep_xview_nucleus_host(orbit._h, C.byref(good), 3, 5, 100, *outs) == L.MBK_OK
    assert p.value >= 1 and n.value >= 0 and 0.5 <= bm.value < 1.0
