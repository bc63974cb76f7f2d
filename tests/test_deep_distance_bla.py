"""Distance estimates for deep views with bilinear approximation on the CPU (include/mbk.h, the section of that name): the
numpy model of the contract (tests/deep_distance_bla_model.py, what the GPU is held to bit for bit) against the truth in mpmath,
its counts against the count model of MBK_DEEP_BLA, the identity with the plain estimate where no level is taken, the host twins
against the model, the derivative skip alone against exact arithmetic, and Koebe's bound.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import deep_bla_model as BL
import deep_distance_bla_model as DB
import deep_distance_model as DD
import deep_model as D
from distributedmandelbrot_amd import DeepOrbit, DeepView, deep_distance_bla_host, deep_distance_bla_skip_host
from distributedmandelbrot_amd import _lib as L
from test_deep_distance import CASES

PICKS = 100
_CACHE = {}


def _case(name):
    """The seeded picks of a 64 x 64 view, as test_deep_distance._case makes them, the table of the full view and the model's
    states on the picks: computed once, shared, left unchanged."""
    if name not in _CACHE:
        centre, span, mrd = CASES[name]
        orbit = DeepOrbit(*centre, mrd, min_span=span)
        view = DeepView(span, 64, 64)
        dr, di = D.offsets(view)
        pick = np.random.RandomState(1).choice(dr.size, PICKS, replace=False)
        zr, zi = orbit.table()
        table = BL.build(zr, zi, BL.dcmax(view))
        st = DB.states(zr, zi, dr[pick], di[pick], mrd, table)
        _CACHE[name] = (orbit, view, pick, dr[pick], di[pick], table, st)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_model_against_truth(name):
    centre, span, mrd = CASES[name]
    orbit, view, pick, dr, di, table, st = _case(name)
    rel = DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"])
    esc = np.flatnonzero(st["n"] > 0)
    assert esc.size >= 0.9 * PICKS, esc.size
    assert len(np.unique(st["n"])) >= 8, np.unique(st["n"])
    errs, agree = [], 0
    for i in esc:
        ok, truth = DD.hp_sample(centre, dr[i], di[i], span, st["n"][i], st["extra"][i], orbit.precision_bits + 128)
        if ok:
            agree += 1
            errs.append(abs(rel[i] - truth) / truth)
    worst = max(errs)
    print(f"{name}: {esc.size} of {PICKS} escaped, {agree} agree in (count, run-on), {len(np.unique(st['n']))} distinct counts, "
          f"e {int(st['e'][esc].min())}..{int(st['e'][esc].max())}, steps executed / iterations "
          f"{st['steps'].sum() / np.where(st['n'] > 0, st['n'], mrd - 1).sum():.3f}, worst relative error of rel {worst:.3e}")
    assert agree >= 0.99 * esc.size, (agree, esc.size)
    assert np.isfinite(rel[esc]).all() and (rel[esc] > 0).all()
    assert worst <= DB.DEEP_BLA_DERIVATIVE_REL, worst
    assert DB.DEEP_BLA_DERIVATIVE_REL <= 1e-4
    assert (st["e"] >= 0).all() and (st["e"] < DD.EXP_CAP).all()


@pytest.mark.parametrize("name", list(CASES))
def test_counts_and_steps_are_the_count_models(name):
    centre, span, mrd = CASES[name]
    orbit, view, pick, dr, di, table, st = _case(name)
    zr, zi = orbit.table()
    c, mg, steps = BL.counts(zr, zi, dr, di, mrd, table)
    assert np.array_equal(st["n"], c) and st["n"].dtype == c.dtype
    assert np.array_equal(st["steps"], steps)


@pytest.mark.parametrize("name", ["i-1e-200", "i-1e-30"])
def test_skips_are_taken(name):
    centre, span, mrd = CASES[name]
    st = _case(name)[6]
    ratio = st["steps"].sum() / np.where(st["n"] > 0, st["n"], mrd - 1).astype(np.int64).sum()
    print(f"{name}: steps executed / reference iterations {ratio:.3f}")
    assert ratio <= 0.5, ratio


def _no_skip_cases():
    # an orbit of length 1 (c = -2 leaves |z| < 2 at its first step: no table; c = 1 + i would have length 2), and the thin
    # view at the root of the period-2 bulb of tests/test_deep_truth.py, whose offsets (|dc_i| >= 3e-5) never pass level 0's
    # radius (~1e-12)
    return {"M == 1": (("-2", "0"), 1e-10, None, 1000), "-0.75 span_i 4e-3": (("-0.75", "0"), 1e-25, 4e-3, 5000)}


@pytest.mark.parametrize("name", list(_no_skip_cases()))
def test_no_skip_identity(name):
    centre, span_r, span_i, mrd = _no_skip_cases()[name]
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i or span_r))
    assert (orbit.length == 1) == (name == "M == 1")
    view = DeepView(span_r, 64, 64, span_i)
    zr, zi = orbit.table()
    dr, di = D.offsets(view)
    table = BL.build(zr, zi, BL.dcmax(view))
    assert (len(table) == 0) == (name == "M == 1")
    st = DB.states(zr, zi, dr, di, mrd, table)
    plain = DD.states(zr, zi, dr, di, mrd)
    assert np.array_equal(st["steps"], np.where(st["n"] > 0, st["n"], mrd - 1))          # no level was ever taken
    assert (st["n"] > 0).any()
    for k in ("n", "extra", "Dr", "Di", "e", "mag", "dmagD"):
        a, b = np.asarray(st[k]), np.asarray(plain[k])
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), k
    rel = DD.value(st["mag"], st["dmagD"], st["e"], span_r, st["n"])
    want = DD.value(plain["mag"], plain["dmagD"], plain["e"], span_r, plain["n"])
    assert np.array_equal(rel.view(np.uint64), want.view(np.uint64))
    # the host twin on a sample of those pixels
    pick = np.random.RandomState(2).choice(dr.size, 40, replace=False)
    got = deep_distance_bla_host(orbit, view, pick, mrd)
    for k in ("n", "extra", "Dr", "Di", "e", "mag", "dmagD", "steps"):
        assert np.array_equal(got[k], st[k][pick]), k
    assert np.array_equal(got["rel"], want[pick])


@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_model(name):
    centre, span, mrd = CASES[name]
    orbit, view, pick, dr, di, table, st = _case(name)
    got = deep_distance_bla_host(orbit, view, pick, mrd)
    for k in ("n", "extra", "mag", "Dr", "Di", "e", "dmagD", "steps"):
        assert np.array_equal(got[k], st[k]), (k, int((got[k] != st[k]).sum()))
    # numpy's ln is glibc's: the model and the host agree to the bit
    assert np.array_equal(got["rel"], DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"]))


def _fl(x: Fraction) -> Fraction:
    """x rounded to the nearest binary64 (ties to even: int / int is correctly rounded), as a Fraction."""
    return Fraction(float(x)) if x else Fraction(0)


def _exact_skip(A, B, Dv, e):
    """The skip rule of the header in exact arithmetic, rounded where the rule rounds: (Dr, Di, e)."""
    ea = math.frexp(max(abs(A[0]), abs(A[1])))[1]
    eb = math.frexp(max(abs(B[0]), abs(B[1])))[1]
    As = [Fraction(a) / Fraction(2) ** ea for a in A]
    Bs = [Fraction(b) / Fraction(2) ** eb for b in B]
    assert all(_fl(x) == x for x in As + Bs)                       # the two scalings are exact
    Dr, Di = Fraction(Dv[0]), Fraction(Dv[1])
    P = (_fl(_fl(As[0] * Dr) - _fl(As[1] * Di)), _fl(_fl(As[0] * Di) + _fl(As[1] * Dr)))
    pe = e + ea
    h = max(pe, eb, 0)
    sp, sb = max(pe - h, -1200), max(eb - h, -1200)
    N = [_fl(_fl(p * Fraction(2) ** sp) + _fl(b * Fraction(2) ** sb)) for p, b in zip(P, Bs)]
    if max(abs(N[0]), abs(N[1])) >= Fraction(2) ** 256:
        N = [_fl(x / Fraction(2) ** 256) for x in N]
        h += 256
    elif max(abs(N[0]), abs(N[1])) < Fraction(1, 2 ** 256) and h >= 256:
        N = [_fl(x * Fraction(2) ** 256) for x in N]
        h -= 256
    return float(N[0]), float(N[1]), min(h, 1 << 30)


BELOW = math.nextafter(2.0 ** 256, 0.0)
SKIPS = {
    "huge A, |D| just below 2^256": ((1e300, -1e299), (1.0, 0.0), (BELOW, -BELOW), 512),
    "tiny A at e = 0": ((1e-300, 0.0), (1.0, 0.0), (1.0, 0.5), 0),
    "huge B at e = 0": ((2.0, 0.0), (1e300, 1e300), (1.0, 0.0), 0),
    "B = 1 vanishes at e = 1100": ((1.5, -0.25), (1.0, 0.0), (3.0, -7.0), 1100),
    "the sum passes 2^256": ((768.0, 768.0), (1.0, 0.0), (BELOW, -BELOW), 256),
    "the sum falls below 2^-256": ((0.5, 0.0), (1.0, 0.0), (2.0 ** -256, -2.0 ** -300), 512),
    "... but e is below 256": ((0.5, 0.0), (0.0, 0.0), (2.0 ** -256, -2.0 ** -300), 255),
    "by hand": ((3.0, 4.0), (1.0, 0.0), (1.0, 0.0), 0),
}


@pytest.mark.parametrize("name", list(SKIPS))
def test_the_skip_alone(name):
    A, B, Dv, e = SKIPS[name]
    want = _exact_skip(A, B, Dv, e)
    host = deep_distance_bla_skip_host(*A, *B, *Dv, e)
    model = DB.skip(*[np.array([x]) for x in (*A, *B, *Dv)], np.array([e]))
    model = (float(model[0][0]), float(model[1][0]), int(model[2][0]))
    print(f"{name}: D = ({want[0]!r}, {want[1]!r}), e = {want[2]}")
    assert all(math.isfinite(x) for x in want[:2]) and 0 <= want[2] < (1 << 30)
    assert max(abs(want[0]), abs(want[1])) < 2.0 ** 256 and (want[2] < 256 or max(abs(want[0]), abs(want[1])) >= 2.0 ** -256)
    for got in (host, model):
        assert np.array_equal(np.array(got[:2]).view(np.uint64), np.array(want[:2]).view(np.uint64)) and got[2] == want[2], (got, want)
    if name == "by hand":
        assert (math.ldexp(want[0], want[2]), math.ldexp(want[1], want[2])) == (4.0, 4.0)
    if name == "B = 1 vanishes at e = 1100":             # d' = A d: the addend is below the subnormals
        assert want[2] == 1101 and want[:2] == (math.ldexp(1.5 * 3.0 - 0.25 * 7.0, -1), math.ldexp(1.5 * -7.0 - 0.25 * 3.0, -1))
    if name == "huge A, |D| just below 2^256":
        assert want[2] == 512 + 997                     # (1e300 = 0.747 2^997: the product stays below 2^256)
    if name == "the sum falls below 2^-256":
        assert want == (0.5, -2.0 ** -45, 256)
    if name == "... but e is below 256":
        assert want == (2.0 ** -257, -2.0 ** -301, 255)
    if name == "the sum passes 2^256":
        assert want[2] == 256 + 10 + 256 and want[0] == math.ldexp(1.5 * BELOW, -256)


def test_a_long_orbit_keeps_the_mantissa_in_range():
    """The seahorse view of scripts/deep_rate.py at 1e-20, mrd 30 000: ~3000 skips per pixel, each of which may move a binade from
    D into e (|As| < 1).  The two-sided rescale keeps max(|Dr|, |Di|) in [2^-256, 2^256), so dmagD cannot underflow and rel is
    finite; with a one-sided rescale D reaches 1e-207 here and rel is inf.  The host twin equals the model on the picks."""
    seahorse = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
    span, mrd, n = 1e-20, 30000, 4096
    orbit = DeepOrbit(*seahorse, mrd, min_span=span)
    view = DeepView(span, n)
    pick = np.random.RandomState(3).choice(n * n, 6, replace=False)
    got = deep_distance_bla_host(orbit, view, pick, mrd)
    top = np.maximum(np.abs(got["Dr"]), np.abs(got["Di"]))
    print(f"n {got['n']}, steps {got['steps']}, e {got['e']}, max(|Dr|, |Di|) {top}, rel {got['rel']}")
    assert (got["n"] > 1000).all() and (got["steps"] < 0.5 * got["n"]).all()
    assert (top >= 2.0 ** -256).all() and (top < 2.0 ** 256).all()
    assert np.isfinite(got["rel"]).all() and (got["rel"] > 0).all() and (got["rel"] < 1).all()
    zr, zi = orbit.table()
    dr, di = D.axis_offsets(n, view.span_r, pick % n), D.axis_offsets(n, view.span_i, pick // n)
    st = DB.states(zr, zi, dr, di, mrd, BL.build(zr, zi, BL.dcmax(view)))
    for k in ("n", "extra", "mag", "Dr", "Di", "e", "dmagD", "steps"):
        assert np.array_equal(got[k], st[k]), k


def test_koebe_bound_at_1e_200():
    """The centre c = i is in the set, so the true distance of a pixel is at most |dc| and de <= 4 |dc|."""
    centre, span, mrd = CASES["i-1e-200"]
    orbit, view, pick, dr, di, table, st = _case("i-1e-200")
    rel = DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"])
    esc = st["n"] > 0
    ratio = rel[esc] / (4.0 * (np.hypot(dr[esc], di[esc]) / span))      # (lengths as fractions of the span: no underflow)
    print(f"largest rel x span / (4 |dc|): {ratio.max():.4f}")
    assert (ratio <= 1.0 + DB.DEEP_BLA_DERIVATIVE_REL).all() and ratio.max() > 0.01


def test_signatures_symbols_and_null_arguments():
    lib = L.load()
    names = ("mbk_deep_view_launch_distance_bla", "mbk_deep_view_compute_distance_bla", "mbk_deep_view_distance_bla_render_launch",
             "mbk_deep_view_distance_bla_render_compute", "mbk_deep_distance_bla_host", "mbk_deep_distance_bla_skip_host")
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mbk_abi_version() == 5
    for name in names[:4]:
        assert getattr(lib, name)(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_distance_bla_skip_host(1.0, 0.0, 1.0, 0.0, None, None, None) == L.MBK_ERR_INVALID
    orbit = DeepOrbit("0", "1", 100, min_span=1e-20)
    view = DeepView(1e-20, 8, 8)
    with pytest.raises(Exception):
        deep_distance_bla_host(orbit, view, [64], 100)                  # a pixel outside the view
    with pytest.raises(Exception):
        deep_distance_bla_host(orbit, view, [0], 101)                   # mrd above the orbit's
    for mrd in (0, 1):
        got = deep_distance_bla_host(orbit, view, np.arange(64), mrd)
        assert not got["n"].any() and not got["rel"].any() and not got["steps"].any()
