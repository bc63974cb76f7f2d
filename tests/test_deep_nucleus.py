"""Locating minibrots in deep views on the CPU (include/mbk.h, "Locating minibrots in deep views"): the host twin of the nucleus
kernel against the numpy model of the contract (tests/deep_nucleus_model.py) bit for bit, the model's atom periods against
mpmath at 1400 bits, the host-only Newton step and size estimate against mpmath at P + 128 bits, refine_nucleus,
pick_nucleus_seed, and locate_nucleus end to end on host-twin arrays.

The three cases, 16 x 16 (found with mpmath before the code was written): c = i at span 1e-20 holds a minibrot of period 56 and
size 5.43e-42, at span 1e-200 one of period 534 and size 1.01e-401 (below 2^-960: found from a DeepView, viewable only as a
WideDeepView); the Misiurewicz point of tests/test_deep_wide.py at span 1e-100 one of period 447 and size 1.08e-201.

Measured here: the separation rule excludes 3, 1 and 0 of the 256 pixels, no well-separated pixel differs; refine_nucleus takes
7, 18 and 13 rounds in locate_nucleus (each round gains the ~51 bits a binary64 Newton step holds); the Newton step's relative
error is at most 0.015 p 2^-48 and the size estimate's at most 0.030 p 2^-48 (the test prints both).
After 1, 13 and 7 polishing rounds the centre strings hold about 370, 2140 and 1160 bits and log2 |z_p| at them is -306.1, -1475.3
and -815.0 against the 40 - P = -280, -1432 and -792 that test_z_p_at_the_result_against_the_bound_of_the_issue asks for.
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
from distributedmandelbrot_amd import (DeepOrbit, DeepView, MbkError, NucleusError, WideDeepView, deep_nucleus_host, locate_nucleus,
                                       pick_nucleus_seed, refine_nucleus)
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import device as dv
from test_deep_wide import MIS

# name: (centre, span, mrd, the period of the minibrot the view holds, its size as a decimal string: one is below binary64)
CASES = {
    "i-1e-20": (("0", "1"), 1e-20, 1500, 56, "5.43e-42"),
    "i-1e-200": (("0", "1"), 1e-200, 4000, 534, "1.01e-401"),
    "mis-1e-100": (MIS, 1e-100, 3000, 447, "1.08e-201"),
}
N = 16
SEPARATION = 2.0 ** -16   # the two smallest |z_n| must differ by more than this share of the smaller
MAX_EXCLUDED = 5


@functools.lru_cache(maxsize=None)
def case(name):
    """(orbit, view, host twin arrays, model arrays) of a case; shared, never modified."""
    centre, span, mrd, _, _ = CASES[name]
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, N, N)
    return orbit, view, deep_nucleus_host(orbit, view, np.arange(N * N), mrd), NM.model(orbit, view, mrd)


@functools.lru_cache(maxsize=None)
def located(name):
    orbit, view, h, _ = case(name)
    return locate_nucleus(orbit, view, CASES[name][2], seeds=(h["period"].reshape(N, N), h["delta"].reshape(N, N, 2)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _truncated(x, P) -> Fraction:
    """x (mpf or Fraction) truncated towards zero at P fraction bits"""
    if not isinstance(x, Fraction):
        sign, man, exp, _ = x._mpf_
        x = (-1 if sign else 1) * Fraction(int(man)) * Fraction(2) ** int(exp)
    t = Fraction((abs(x.numerator) << P) // x.denominator, 1 << P)
    return -t if x < 0 else t


def _mpc_wide(r, i, e):
    return mpmath.mpc(mpmath.ldexp(mpmath.mpf(r), e), mpmath.ldexp(mpmath.mpf(i), e))


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_model_bit_for_bit(name):
    orbit, view, h, st = case(name)
    for key in ("n", "period", "best", "z", "D", "e", "delta"):
        assert h[key].shape == st[key].shape, key
        assert np.array_equal(_bits(h[key]), _bits(st[key])), (name, key, int((_bits(h[key]) != _bits(st[key])).sum()))
    counts, _ = D.model_counts(*orbit.table(), *D.offsets(view), CASES[name][2])
    assert np.array_equal(h["n"], counts)
    assert np.isfinite(h["delta"]).all() and (h["period"] >= 1).all()
    if name == "i-1e-200":
        assert (h["e"] >= 512).all()      # |d| ~ 1e200: the kept derivative has been rescaled


@pytest.mark.parametrize("centre,span,mrds", [(("-2", "0"), 1e-10, (1000,)),          # M == 1: the reference escapes at once
                                              (("0.26", "0"), 0.05, (300,)),          # the orbit runs out: rebases at m == M
                                              (("0", "1"), 1e-20, (0, 1, 2, 40))])    # no step, one step, mrd below the period
def test_host_twin_equals_the_model_on_the_edges(centre, span, mrds):
    orbit = DeepOrbit(*centre, max(max(mrds), 2), min_span=span)
    view = DeepView(span, 19, 13)
    for mrd in mrds:
        h, st = deep_nucleus_host(orbit, view, np.arange(19 * 13), mrd), NM.model(orbit, view, mrd)
        for key in st:
            assert np.array_equal(_bits(h[key]), _bits(st[key])), (centre, mrd, key)
        assert h["period"].max() <= max(mrd, 1)


@pytest.mark.parametrize("name", list(CASES))
def test_model_period_is_mpmaths_argmin(name):
    centre, span, mrd, _, _ = CASES[name]
    _, view, _, st = case(name)
    dcr, dci = D.offsets(view)
    excluded, wrong = 0, []
    for j in range(N * N):
        arg, first, second = NM.hp_argmin(centre, dcr[j], dci[j], mrd)
        with mpmath.workprec(NM.TRUTH_BITS):
            a, b = mpmath.sqrt(first), mpmath.sqrt(second)
            separated = b - a > SEPARATION * a
        if not separated:
            excluded += 1
        elif arg + 1 != st["period"][j]:
            wrong.append((j, arg + 1, int(st["period"][j])))
    print(f"{name}: {excluded} of {N * N} pixels excluded by the separation rule, {len(wrong)} well-separated pixels differ")
    assert excluded <= MAX_EXCLUDED, excluded
    assert not wrong, wrong[:5]


def _basic_nuclei():
    """(name, binary64 seed, period, P)"""
    return [("airplane", (-1.7548776662466927, 0.0), 3, 256), ("rabbit", (-0.12256116687665362, 0.7448617666197442), 3, 256),
            ("real period 5", (-1.6254137251233037, 0.0), 5, 256)]


@pytest.mark.parametrize("which", ["airplane", "rabbit", "real period 5"] + list(CASES))
def test_newton_step_and_size_against_mpmath(which):
    """The size is taken at the nucleus (truncated to P bits, as the library reads it).  The Newton step is compared at the
    nucleus truncated to P / 2 bits: at the nucleus itself Z_p is nothing but the fixed-point orbit's truncation noise (of the
    order of p 2^-P), so there only its magnitude is held, to the convergence bound 2^(32 - P)."""
    if which in CASES:
        nuc = located(which)
        seed, p, P = (dv._exact_fraction(nuc.center_r), dv._exact_fraction(nuc.center_i)), nuc.period, nuc.precision_bits
    else:
        seed, p, P = next(((Fraction(s[0]), Fraction(s[1])), p, P) for n, s, p, P in _basic_nuclei() if n == which)
    root = NM.hp_newton(seed[0], seed[1], p, P + 128)
    bound = p * 2.0 ** -48
    with mpmath.workprec(P + 128):
        full = (_truncated(root.real, P), _truncated(root.imag, P))
        o = DeepOrbit(dv._dyadic_decimal(full[0]), dv._dyadic_decimal(full[1]), p + 1, precision_bits=P)
        assert o.length == p + 1
        _, want = NM.hp_step_and_size(NM.mpc_of(*full), p)
        got = _mpc_wide(*dv.orbit_size_host(o, p))
        err_size = float(abs(got - want) / abs(want))
        step = _mpc_wide(*dv.orbit_newton_host(o, p))
        assert abs(step) <= mpmath.ldexp(1, 32 - P), float(mpmath.log(abs(step), 2))
        half = (_truncated(root.real, P // 2), _truncated(root.imag, P // 2))
        o2 = DeepOrbit(dv._dyadic_decimal(half[0]), dv._dyadic_decimal(half[1]), p + 1, precision_bits=P)
        want, _ = NM.hp_step_and_size(NM.mpc_of(*half), p)
        got = _mpc_wide(*dv.orbit_newton_host(o2, p))
        err_step = float(abs(got - want) / abs(want))
        # the step leads back to the root: what is left is of second order
        assert abs(NM.mpc_of(*half) + got - root) <= abs(want) * mpmath.mpf(2) ** -40
    print(f"{which}: p {p}, P {P}: Newton step rel. error {err_step / bound:.3f} p 2^-48, size {err_size / bound:.3f} p 2^-48")
    assert err_step <= bound and err_size <= bound, (err_step, err_size, bound)
    if which in CASES:
        size = abs(_mpc_wide(nuc.size_r, nuc.size_i, nuc.size_e))
        with mpmath.workprec(64):
            assert abs(size / mpmath.mpf(CASES[which][4]) - 1) < 0.01


def test_period_one_and_refusals():
    o = DeepOrbit("0", "0", 4, precision_bits=64)
    assert dv.orbit_size_host(o, 1) == (0.5, 0.0, 1)        # exactly 1
    assert dv.orbit_newton_host(o, 1)[:2] == (0.0, 0.0)     # Z_1 = 0: c = 0 is the period-1 nucleus
    lib = L.load()
    r, i, e = C.c_double(-7.0), C.c_double(-7.0), C.c_int32(-7)
    for fn in (lib.mbk_deep_orbit_newton_host, lib.mbk_deep_orbit_size_host):
        assert fn(o._h, 5, C.byref(r), C.byref(i), C.byref(e)) == L.MBK_ERR_INVALID      # the orbit is shorter than the period
        assert fn(o._h, 0, C.byref(r), C.byref(i), C.byref(e)) == L.MBK_ERR_INVALID
        assert fn(None, 1, C.byref(r), C.byref(i), C.byref(e)) == L.MBK_ERR_INVALID
        assert fn(o._h, 1, None, C.byref(i), C.byref(e)) == L.MBK_ERR_INVALID
    assert (r.value, i.value, e.value) == (-7.0, -7.0, -7)
    esc = DeepOrbit("1", "1", 50, precision_bits=64)       # escapes after a few steps
    assert esc.escaped and fn(esc._h, 40, C.byref(r), C.byref(i), C.byref(e)) == L.MBK_ERR_INVALID
    with pytest.raises(ValueError):
        deep_nucleus_host(o, WideDeepView(0.5, -1000, 4, 4), [0], 4)
    with pytest.raises(MbkError):
        deep_nucleus_host(o, DeepView(1e-3, 4, 4), [0], 5)  # mrd above the orbit's


def test_refine_nucleus():
    nuc = located("i-1e-20")
    P, p = nuc.precision_bits, nuc.period
    seed = (dv._exact_fraction(nuc.center_r), dv._exact_fraction(nuc.center_i))
    root = NM.hp_newton(seed[0], seed[1], p, P + 128)
    with mpmath.workprec(P + 128):
        half = (_truncated(root.real, P // 2), _truncated(root.imag, P // 2))   # half its digits
        assert abs(NM.mpc_of(*half) - root) > mpmath.ldexp(1, -P // 2 - 2)
        for start_period in (p, 2 * p):
            got = refine_nucleus(half[0], half[1], start_period, P)
            assert got.period == p and got.precision_bits == P and got.seed_pixel is None and 1 <= got.rounds <= 8
            c = NM.mpc_of(dv._exact_fraction(got.center_r), dv._exact_fraction(got.center_i))
            assert abs(c - root) <= mpmath.ldexp(1, 32 - P), float(mpmath.log(abs(c - root), 2))
            assert abs(got.size_log2 - nuc.size_log2) < 1e-9
    # a decimal string is read exactly: the same seed, the same result
    again = refine_nucleus(dv._dyadic_decimal(half[0]), dv._dyadic_decimal(half[1]), 2 * p, P)
    assert again == got
    with pytest.raises(NucleusError) as e:
        refine_nucleus(half[0], half[1], p, 128)            # size 2^-137: 201 bits are needed
    assert e.value.reason == "precision" and "precision" in str(e.value)
    with pytest.raises(NucleusError) as e:
        refine_nucleus(half[0], half[1], p, P, max_rounds=1)
    assert e.value.reason == "not converged"
    with pytest.raises(NucleusError) as e:
        refine_nucleus("1", "1", 7, 128)                    # the orbit of 1 + i escapes before step 7
    assert e.value.reason == "not converged"


def test_pick_nucleus_seed_on_hand_made_arrays():
    view = DeepView(1.0, 5, 5)                              # pixel offsets -0.5, -0.25, 0, 0.25, 0.5 on both axes
    period = np.full((5, 5), 9, np.int32)
    delta = np.zeros((5, 5, 2))
    delta[..., 0] = 0.125
    delta[:, 4, 0] = 0.001                                  # column 4: 0.5 + 0.001 is out of view
    # nothing special: every in-view pixel has period 9 and |delta| 0.125: the first in image order
    s = pick_nucleus_seed(view, period, delta)
    assert s.pixel == (0, 0) and s.period == 9 and (s.offset_r, s.offset_i) == (Fraction(-3, 8), Fraction(-1, 2))
    # the lowest period wins over a smaller |delta|
    period[3, 1] = 4
    delta[2, 2] = (0.01, 0.0)
    s = pick_nucleus_seed(view, period, delta)
    assert s.pixel == (3, 1) and s.period == 4 and (s.offset_r, s.offset_i) == (Fraction(-1, 8), Fraction(1, 4))
    # ... unless its target is out of view, or its delta is inf
    delta[3, 1] = (0.9, 0.0)
    assert pick_nucleus_seed(view, period, delta).pixel == (2, 2)
    delta[3, 1] = (np.inf, np.inf)
    period[0, 4] = 2                                        # out of view (column 4)
    assert pick_nucleus_seed(view, period, delta).pixel == (2, 2)
    # among equal periods the smallest |delta|, then image order
    delta[2, 2] = (0.125, 0.0)
    delta[1, 3] = (0.0, -0.0625)
    delta[4, 0] = (0.0625, 0.0)
    assert pick_nucleus_seed(view, period, delta).pixel == (1, 3)
    # a target exactly on the edge is in view; one ulp beyond is not
    edge = np.full((5, 5, 2), np.inf)
    edge[2, 3] = (0.25, 0.0)
    assert pick_nucleus_seed(view, period, edge).pixel == (2, 3)
    edge[2, 3] = (np.nextafter(0.25, 1.0), 0.0)
    assert pick_nucleus_seed(view, period, edge) is None
    # nothing in view
    assert pick_nucleus_seed(view, period, np.full((5, 5, 2), np.inf)) is None
    assert pick_nucleus_seed(view, period, np.full((5, 5, 2), 3.0)) is None


def _count_host(orbit, view, col, row, mrd):
    if isinstance(view, WideDeepView):
        cv = dv._cxview(view)
        n, mag = C.c_int32(), C.c_double()
        assert L.load().mbk_deep_xview_count_host(orbit._h, C.byref(cv), col, row, mrd, C.byref(n), C.byref(mag)) == L.MBK_OK
        return n.value
    return int(deep_nucleus_host(orbit, view, [row * view.width + col], mrd)["n"][0])


@pytest.mark.parametrize("name", list(CASES))
def test_locate_nucleus_end_to_end_on_host_twin_arrays(name):
    centre, span, mrd, period, size = CASES[name]
    orbit, view, _, _ = case(name)
    nuc = located(name)
    P = nuc.precision_bits
    assert nuc.period == period and nuc.inside and nuc.seed_pixel is not None
    assert P == dv.nucleus_precision_bits(view) == -(-math.ceil(2 * -math.log2(span) + 128) // 64) * 64
    print(f"{name}: period {nuc.period}, {nuc.rounds} rounds at {P} bits, |size| 2^{nuc.size_log2:.2f}, seed pixel {nuc.seed_pixel}")
    # mpmath, on its own: the result is within 2^(40 - P) of a root of z_p (|z_p / d_p|, the distance to first order; |z_p| itself:
    # test_z_p_at_the_result_against_the_bound_of_the_issue) and no proper divisor's z vanishes there
    with mpmath.workprec(P + 128):
        c = NM.mpc_of(dv._exact_fraction(nuc.center_r), dv._exact_fraction(nuc.center_i))
        tiny = mpmath.ldexp(1, 40 - P)
        step, _ = NM.hp_step_and_size(c, period)
        assert abs(step) <= tiny
        for q in range(1, period):
            if period % q == 0:
                assert abs(NM.hp_z(c, q)) > tiny, q
        off = c - NM.mpc_of(D.exact(centre[0]), D.exact(centre[1]))
        assert abs(off.real) <= span / 2 and abs(off.imag) <= span / 2
    # the view it frames: the nucleus in the middle, the corners outside the minibrot
    v = nuc.view(17, 17)
    assert isinstance(v, WideDeepView if 4 * D.exact(size) < Fraction(2) ** -960 else DeepView)
    mrd2 = 16 * period
    o = nuc.orbit(mrd2)
    assert o.length == mrd2 and o.precision_bits == P
    assert _count_host(o, v, 8, 8, mrd2) == 0
    for col, row in ((0, 0), (16, 0), (0, 16), (16, 16)):
        assert _count_host(o, v, col, row, mrd2) > 0, (col, row)


@pytest.mark.parametrize("name", list(CASES))
def test_z_p_at_the_result_against_the_bound_of_the_issue(name):
    """The check as the issue states it: mpmath confirms |z_p| <= 2^(40 - P) at the result.

    No centre on the 2^-P grid can pass it: to first order |z_p(C)| = |d_p| |C - nucleus|, the grid point nearest to the nucleus is
    generically ~2^-P away, and |d_p| ~ 1 / sqrt(size) of a minibrot is far above 2^40 (here 2^68.5, 2^666.0 and 2^333.4; a centre
    good to its last place at P bits measured log2 |z_p| = -251.6, -808.3 and -498.4 against 40 - P = -280, -1432 and -792).  That
    is what refine_nucleus' polishing phase is for: the centre strings carry P + log2(1 / sqrt(size)) + 64 bits.  mpmath works
    at 128 bits more than the strings hold, so that it reads them exactly."""
    nuc = located(name)
    P, p = nuc.precision_bits, nuc.period
    Cr, Ci = dv._exact_fraction(nuc.center_r), dv._exact_fraction(nuc.center_i)
    held = max(Cr.denominator.bit_length(), Ci.denominator.bit_length())
    assert P < held <= 4097 and nuc.polish_rounds >= 1
    with mpmath.workprec(max(P, held) + 128):
        c = NM.mpc_of(Cr, Ci)
        z, d = c, mpmath.mpc(1)
        for _ in range(p - 1):
            d = 2 * z * d + 1
            z = z * z + c
        lz, ld = float(mpmath.log(abs(z), 2)), float(mpmath.log(abs(d), 2))
        print(f"{name}: log2 |z_p| {lz:.1f} against 40 - P = {40 - P}; log2 |d_p| {ld:.1f}; log2 |z_p / d_p| {lz - ld:.1f}")
        assert abs(z) <= mpmath.ldexp(1, 40 - P), (lz, 40 - P)


def test_locate_nucleus_refuses_wide_views_and_empty_seeds():
    orbit, view, h, _ = case("i-1e-20")
    with pytest.raises(ValueError):
        locate_nucleus(orbit, WideDeepView(0.5, -1000, N, N), 1500, seeds=(h["period"].reshape(N, N), h["delta"].reshape(N, N, 2)))
    with pytest.raises(NucleusError) as e:
        locate_nucleus(orbit, view, 1500, seeds=(h["period"].reshape(N, N), np.full((N, N, 2), np.inf)))
    assert e.value.reason == "no seed"
