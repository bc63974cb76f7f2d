"""Distance estimates for extended-range deep views on the CPU (include/mbk.h, the section of that name): the host twins
against the numpy model (tests/deep_wide_distance_model.py) bit for bit, the model against d' = 2 z d + 1 in mpmath at
P + 128 bits, against the plain deep distance model wherever a plain view can name the spans, the derivative step on
synthetic operands against exact rational arithmetic, Koebe's bound, the output rule, the palette helpers and the refusals.
No GPU."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import deep_distance_model as DD
import deep_model as D
import deep_wide_distance_model as WD
import deep_wide_model as W
from distributedmandelbrot_amd import DeepOrbit, DeepView, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import device as DEV
from test_deep_wide import SAME, TRUTH_CASES, _sample

IDS = [c[-1] for c in TRUTH_CASES]
_STATES = {}


def _states(centre, rng, exp2, mrd, bits, key):
    """The case's sample (test_deep_wide._sample: orbit, view, 150 seeded picks) and the model's states on it, computed once."""
    orbit, view, pick, dr, di, count, _ = _sample(centre, rng, exp2, mrd, bits, key)
    if key not in _STATES:
        st = WD.states(*orbit.wide_table(), dr, di, exp2, mrd)
        for a in st.values():
            a.setflags(write=False)
        assert np.array_equal(st["n"], count)          # the count is exactly the wide count
        _STATES[key] = st
    return orbit, view, pick, dr, di, _STATES[key]


def _assert_twin_equals(host, st, view, what):
    for k in ("n", "extra", "e"):
        assert np.array_equal(host[k], st[k]), (what, k, int((host[k] != st[k]).sum()))
    for k in ("mag", "Dr", "Di", "dmagD"):
        assert np.array_equal(host[k].view(np.uint64), st[k].view(np.uint64)), (what, k)
    return WD.assert_states_agree(host["rel"], st, view.range_r, view.exp2, what)


# ---- host twin == model ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_host_twin_equals_the_model(centre, rng, exp2, mrd, bits, key):
    orbit, view, pick, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    host = DEV.wide_distance_host(orbit, view, pick, mrd)
    share = _assert_twin_equals(host, st, view, key)
    esc = st["n"] > 0
    print(f"{key}: {int(esc.sum())} of {pick.size} escaped, e {int(st['e'][esc].min())}..{int(st['e'][esc].max())}, "
          f"run-on {int(st['extra'][esc].min())}..{int(st['extra'][esc].max())}, host ln == numpy ln on {share:.3f}")
    assert (st["mag"][esc] >= 4.0).all() and not st["mag"][~esc].any()
    assert ((st["mag"][esc] >= WD.RADIUS2) | (st["extra"][esc] == WD.RUN_ON)).all()


def test_m_equals_one_host_twin_equals_the_model():
    """Centre -2: the orbit escapes at M = 1 and every step rebases."""
    mrd, exp2 = 400, -1100
    view = WideDeepView(1.0, exp2, 24, 20)
    orbit = DeepOrbit("-2", "0", mrd, min_span_exp2=view.min_span_exp2)
    assert orbit.length == 1 and orbit.escaped
    rel, n, st = WD.model(orbit, view, mrd)
    assert np.array_equal(n.ravel(), W.model_counts(*orbit.wide_table(), *W.offsets(view), exp2, mrd)[0])
    host = DEV.wide_distance_host(orbit, view, np.arange(n.size), mrd)
    _assert_twin_equals(host, st, view, "M == 1")
    assert (n > 0).sum() > n.size // 2 and np.isfinite(rel).all()


# ---- model == truth -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_model_against_truth(centre, rng, exp2, mrd, bits, key):
    """The first 100 of the sample's 150 picks; the first 40 at exp2 = -3000, where 100 take most of a minute of mpmath
    (measured once at 100 too: deep_wide_distance_model.MEASURED_REL).  Every escaped pick agrees in (count, run-on) on every
    case."""
    orbit, view, pick, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    picks = 40 if exp2 == -3000 else 100
    deep = key != "1e-400"
    rel = WD.value(st["mag"], st["dmagD"], st["e"], rng, exp2, st["n"])[:picks]
    n = st["n"][:picks]
    esc = np.flatnonzero(n > 0)
    errs, agree = [], 0
    for i in esc:
        ok, truth = WD.hp_sample(centre, dr[i], di[i], rng, exp2, n[i], st["extra"][i], orbit.precision_bits + 128)
        if ok:
            agree += 1
            errs.append(abs(rel[i] - truth) / truth)
    worst = max(errs)
    distinct = len(np.unique(n))
    print(f"{key}: {esc.size} of {picks} escaped, {agree} agree in (count, run-on), {distinct} distinct counts "
          f"{n[esc].min()}..{n[esc].max()}, e {int(st['e'][:picks][esc].min())}..{int(st['e'][:picks][esc].max())}, "
          f"worst relative error of rel {worst:.3e}")
    assert agree >= 0.99 * esc.size, (agree, esc.size)
    assert esc.size >= (0.9 if deep else 0.8) * picks, esc.size
    assert distinct >= (8 if deep else 5), np.unique(n)
    assert np.isfinite(rel[esc]).all() and (rel[esc] > 0).all()
    assert worst <= WD.WIDE_DERIVATIVE_REL, worst


def test_the_tolerance_follows_the_rule():
    """The worst measured, one digit rounded up, times 4; and never wider than 1e-4."""
    worst = max(WD.MEASURED_REL.values())
    digit = 10.0 ** math.floor(math.log10(worst))
    assert set(WD.MEASURED_REL) == set(IDS)
    assert math.isclose(WD.WIDE_DERIVATIVE_REL, 4 * math.ceil(worst / digit - 1e-9) * digit, rel_tol=1e-12)
    assert WD.WIDE_DERIVATIVE_REL <= 1e-4


# ---- a wide view of plain spans stores what the plain view stores ------------------------------------------------------

def _assert_wide_equals_plain(centre, span_r, span_i, mrd, width, height):
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i))
    plain = DeepView(span_r, width, height, span_i)
    pst = DD.states(*orbit.table(), *D.offsets(plain), mrd)
    prel = DD.value(pst["mag"], pst["dmagD"], pst["e"], span_r, pst["n"])
    rr, ri, exp2 = W.as_wide(span_r, span_i)
    assert np.ldexp(rr, exp2) == span_r and np.ldexp(ri, exp2) == span_i
    view = WideDeepView(rr, exp2, width, height, ri)
    wrel, wn, wst = WD.model(orbit, view, mrd)
    assert np.array_equal(wst["n"], pst["n"]), int((wst["n"] != pst["n"]).sum())
    assert np.array_equal(wst["extra"], pst["extra"]), int((wst["extra"] != pst["extra"]).sum())
    assert np.array_equal(wrel.ravel().view(np.uint64), prel.view(np.uint64)), int((wrel.ravel() != prel).sum())
    esc = pst["n"] > 0
    # D 2^e is the plain contract's number
    for k in ("Dr", "Di"):
        assert np.array_equal(np.ldexp(wst[k][esc], (wst["e"][esc] - pst["e"][esc]).astype(np.int32)), pst[k][esc]), k
    return orbit, view, wst, int(pst["e"].max())


@pytest.mark.parametrize("centre, span_r, span_i, mrd, M, escaped", SAME, ids=[c[0][0][:12] + "@%g" % c[1] for c in SAME])
def test_wide_model_equals_the_plain_model(centre, span_r, span_i, mrd, M, escaped):
    """No value of these plain runs is subnormal: n, the run-on length and rel are equal bit for bit on the whole 64 x 64
    view -- no case is excused -- and the host twin equals both on a sample."""
    orbit, view, wst, _ = _assert_wide_equals_plain(centre, span_r, span_i or span_r, mrd, 64, 64)
    assert (orbit.length, orbit.escaped) == (M, escaped)
    pick = np.random.RandomState(1).choice(wst["n"].size, 60, replace=False)
    host = DEV.wide_distance_host(orbit, view, pick, mrd)
    _assert_twin_equals(host, {k: v[pick] for k, v in wst.items()}, view, "catalogue")


@pytest.mark.parametrize("span, top", [(1e-200, 512), (1e-280, 768), (2.0 ** -960, 768)], ids=["1e-200", "1e-280", "2^-960"])
def test_wide_model_equals_the_plain_model_where_it_rescales(span, top):
    """c = i, 24 x 20, equal spans on both axes: the plain derivative is rescaled up to e = `top`."""
    _, _, wst, emax = _assert_wide_equals_plain(("0", "1"), span, span, 3000, 24, 20)
    assert emax == top and (wst["n"] > 0).mean() > 0.9


# ---- the derivative step on synthetic operands -------------------------------------------------------------------------

def _ref_dstep(zr, zi, t, Dr, Di, e):
    """The step in exact rational arithmetic, each operation rounded once (float(Fraction) rounds to nearest-even, subnormals
    included)."""
    F = Fraction

    def sh(x, k):
        return float(F(x) * F(2) ** max(k, -1200))

    p0, p1, p2, p3 = (float(F(a) * F(b)) for a, b in ((zr, Dr), (zi, Di), (zr, Di), (zi, Dr)))
    Pr, Pi = float(F(p0) - F(p1)), float(F(p2) + F(p3))
    pe = t + e + 1
    h = max(pe, 0)
    Nr, Ni = float(F(sh(Pr, pe - h)) + F(sh(1.0, -h))), sh(Pi, pe - h)
    mx = max(abs(Nr), abs(Ni))
    if mx == 0.0:
        return 0.0, 0.0, W.EZ
    s = math.frexp(mx)[1]
    return float(F(Nr) / F(2) ** s), float(F(Ni) / F(2) ** s), min(h + s, 1 << 30)


def _both_steps(zr, zi, t, Dr, Di, e):
    host = DEV.wide_distance_step_host(zr, zi, t, Dr, Di, e)
    with np.errstate(all="ignore"):
        m = WD.dstep(np.array([zr]), np.array([zi]), np.array([t], np.int64), np.array([Dr]), np.array([Di]), np.array([e], np.int64))
    model = (float(m[0][0]), float(m[1][0]), int(m[2][0]))
    want = _ref_dstep(zr, zi, t, Dr, Di, e)
    # the twin and the model bit for bit; the rationals by value (they have no signed zero)
    assert [np.float64(v).view(np.uint64) for v in host[:2]] == [np.float64(v).view(np.uint64) for v in model[:2]], (host, model)
    assert host == model == want, (host, model, want, (zr, zi, t, Dr, Di, e))
    return want


def test_derivative_step_on_synthetic_operands():
    # the product a binary64 zp would lose: |zp| ~ 2^-1500, |d| ~ 2^1490
    Dr, Di, e = _both_steps(0.7, -0.3, -1500, 0.6, 0.9, 1490)
    assert e == 1 and (Dr, Di) != (0.5, 0.0) and abs(Dr - 0.5) < 2.0 ** -8          # 1 + 2 zp d, |2 zp d| ~ 2^-9
    assert math.ldexp(0.7, -1500) == 0.0                                             # (what binary64 makes of that zp)
    # P is dropped and D = 1
    assert _both_steps(0.7, -0.3, -1500, 0.6, 0.9, 0) == (0.5, 0.0, 1)
    # pe = 1300: the +1 is dropped
    Dr, Di, e = _both_steps(0.9, 0.2, 0, 0.6, -0.8, 1299)
    assert e in (1300, 1301) and (Dr, Di) == tuple(math.ldexp(v, 1300 - e) for v in (0.9 * 0.6 - 0.2 * -0.8, 0.9 * -0.8 + 0.2 * 0.6))
    # zp = 0
    assert _both_steps(0.0, 0.0, W.EZ, 0.6, 0.9, 5) == (0.5, 0.0, 1)
    # a zero D comes back as 1
    assert _both_steps(0.7, -0.3, 2, 0.0, 0.0, W.EZ) == (0.5, 0.0, 1)
    # e at the cap: it stays there
    assert _both_steps(0.9, 0.1, 3, 0.6, 0.9, 1 << 30)[2] == 1 << 30
    assert _both_steps(0.9, 0.1, -3, 0.6, 0.9, 1 << 30)[2] == (1 << 30) - 2 + math.frexp(0.9 * 0.9 + 0.1 * 0.6)[1]
    # P cancels the 1 exactly: a zero D is (0, 0, EZ)
    assert _both_steps(-1.0, 0.0, 0, 0.5, 0.0, 0) == (0.0, 0.0, W.EZ)
    # e may decrease
    assert _both_steps(0.5, 0.0, -40, 0.5, 0.0, 30)[2] == 1
    # seeded operands around every alignment, the subnormal shifts of sh included
    rs = np.random.RandomState(7)
    for _ in range(400):
        zr, zi, Dr, Di = (float(v) for v in rs.uniform(-1, 1, 4))
        if rs.rand() < 0.5:
            Dr = math.copysign(rs.uniform(0.5, 1), Dr)
        else:
            Di = math.copysign(rs.uniform(0.5, 1), Di)
        e = int(rs.randint(-30, 1400))
        t = int(rs.choice([-e - 1, -e + int(rs.randint(-60, 60)), -e - 1 - int(rs.randint(1000, 1300)), int(rs.randint(-1500, 20))]))
        _both_steps(zr, zi, t, Dr, Di, e)


# ---- smaller checks ----------------------------------------------------------------------------------------------------

def test_koebe_bound_at_exp2_minus_1100():
    """The centre c = i is in the set, so the true distance of a pixel is at most |dc| and de <= 4 |dc|."""
    centre, rng, exp2, mrd, bits, key = TRUTH_CASES[0]
    assert key == "i-1100"
    _, _, _, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    rel = WD.value(st["mag"], st["dmagD"], st["e"], rng, exp2, st["n"])
    esc = st["n"] > 0
    ratio = rel[esc] / (4.0 * (np.hypot(dr[esc], di[esc]) / rng))      # (lengths as fractions of the span)
    print(f"largest rel x span / (4 |dc|): {ratio.max():.4f}")
    assert (ratio <= 1.0 + WD.WIDE_DERIVATIVE_REL).all() and ratio.max() > 0.01


def test_output_rule_special_values():
    v = DEV.wide_distance_value_host
    assert v(1e10, 1.0, 1500, 1.5, -1100, 0) == 0.0
    assert v(1e10, 1.0, 1500, 1.5, -1100, -3) == 0.0
    assert v(1e10, 0.0, W.EZ, 1.5, -1100, 5) == math.inf
    assert v(1e10, math.nan, 0, 1.0, -20, 5) == 0.0
    assert v(math.nan, 1.0, 0, 1.0, -20, 5) == 0.0
    assert v(math.inf, math.inf, 0, 1.0, -20, 5) == 0.0
    # the exponents add up exactly: the same mantissa at every (e, range_r, exp2)
    base = v(1e10, 1.25, 0, 0.75, 0, 7)
    assert base > 0
    for e, k, exp2 in ((1101, 0, -1100), (3005, 2, -3000), (8000, -64, -8192), (-7, 1, 0), (1 << 20, 0, -8192)):
        assert v(1e10, 1.25, e, math.ldexp(0.75, k), exp2, 7) == math.ldexp(base, -(e + k + exp2)), (e, k, exp2)
    # what the plain rule gives for the same numbers
    assert v(1e10, 1.25, 300, 0.75, -200, 7) == L.load().mbk_deep_distance_value_host(1e10, 1.25, 300, math.ldexp(0.75, -200), 7)
    # an e large enough that rel is 0, and the cap
    assert v(1e10, 1.25, 3000, 0.75, -1100, 7) == 0.0
    assert v(1e10, 1.25, 1 << 30, 0.75, -8192, 7) == 0.0
    # the model's rule on the same values
    for args in ((1e10, 1.25, 1101, 0.75, -1100, 7), (1e10, 0.0, W.EZ, 1.5, -1100, 5), (1e10, 1.25, 1 << 30, 0.75, -8192, 7),
                 (1e10, 1.25, 2170, 0.75, -1100, 7), (math.nan, 1.0, 0, 1.0, -20, 5), (1e10, 1.0, 0, 1.0, -20, 0)):
        mag, dm, e, r, x, n = args
        want = WD.value(np.array([mag]), np.array([dm]), np.array([e]), r, x, np.array([n]))[0]
        assert np.float64(v(*args)).view(np.uint64) == np.float64(want).view(np.uint64), args
    assert 0.0 < v(1e10, 1.25, 2170, 0.75, -1100, 7) < 2.0 ** -1022         # a subnormal result rounds once (checked above)


def test_palette_helpers_take_a_wide_view():
    """Only the width enters: the palette of a WideDeepView is the palette of a DeepView of the same width."""
    wide, plain = WideDeepView(1.5, -3000, 801, 601), DeepView(1e-250, 801, 601)
    for kw in (dict(), dict(inner_px=1.0), dict(inner_px=0.5, n=64)):
        a, b = Palette.deep_distance(wide, 8.0, **kw), Palette.deep_distance(plain, 8.0, **kw)
        assert (a.scale, a.offset) == (b.scale, b.offset) and np.array_equal(a.entries, b.entries)
    assert Palette.deep_distance(wide, 8.0, inner_px=1.0).scale == 255 * 800 / 7.0
    base = Palette(np.zeros((10, 4), np.uint8))
    assert base.for_deep_distance(wide, 3.0).scale == 9 * 800 / 3.0 and base.for_deep_distance(wide, 3.0).offset == 0.0
    # a single column: the rows' pitch in units of the real span, the common 2^exp2 cancelled
    col = WideDeepView(1.0, -2000, 1, 11, 2.0)
    assert base.for_deep_distance(col, 3.0).scale == base.for_deep_distance(DeepView(1e-30, 1, 11, 2e-30), 3.0).scale == 9 * 10 * 0.5 / 3.0


def test_signatures_and_symbols():
    lib = L.load()
    names = ("mbk_deep_xview_launch_distance", "mbk_deep_xview_compute_distance", "mbk_deep_xview_distance_render_launch",
             "mbk_deep_xview_distance_render_compute", "mbk_deep_xview_distance_host", "mbk_deep_xdistance_step_host",
             "mbk_deep_xdistance_value_host")
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.mbk_abi_version() == 5
    assert C.sizeof(L.mbk_deep_xview) == 2 * 8 + 7 * 4 + 4
    for name in names[:2]:
        assert getattr(lib, name)(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
        assert L.SIGNATURES[name][1] == L.SIGNATURES[name.replace("xview", "view")][1][:2] + [C.POINTER(L.mbk_deep_xview)] + \
            L.SIGNATURES[name.replace("xview", "view")][1][3:]
    for name in names[2:4]:
        assert getattr(lib, name)(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
        assert L.SIGNATURES[name] == L.SIGNATURES[name.replace("_distance_render_", "_render_")]
    assert L.SIGNATURES["mbk_deep_xdistance_value_host"][0] is C.c_double
    assert lib.mbk_deep_xdistance_step_host(0.5, 0.5, 0, None, None, None) == L.MBK_ERR_INVALID
    from distributedmandelbrot_amd import MandelbrotDevice
    for name in ("compute_wide_view_distance", "launch_wide_view_distance", "render_wide_view_distance",
                 "launch_render_wide_view_distance"):
        assert callable(getattr(MandelbrotDevice, name))


WIDE_RANGE = "extended-range deep view ranges must be finite and lie in [2^-64, 4]"
WIDE_EXP2 = "extended-range deep view exp2 must lie in [-8192, 0]"
# (what differs from a served call, the message); orbit mrd 100, view 16 x 16 of span 2^-50, pixel (3, 4), mrd 50
REFUSALS = [
    (dict(orbit=None), "orbit is NULL"),
    (dict(view=None), "view is NULL"),
    (dict(out=None), "NULL argument"),
    (dict(width=0), "empty view"),
    (dict(ncols=0), "empty window"),
    (dict(col0=10, ncols=7), "window exceeds the view"),
    (dict(width=1 << 16, height=1 << 16, ncols=1 << 16, nrows=(1 << 15) + 1), "window larger than 2^31 pixels"),
    (dict(range_r=2.0 ** -65), WIDE_RANGE),
    (dict(range_i=float("inf")), WIDE_RANGE),
    (dict(exp2=1), WIDE_EXP2),
    (dict(exp2=-8193), WIDE_EXP2),
    (dict(mrd=101), "mrd exceeds the mrd the reference orbit was computed for"),
    (dict(col=16), "pixel outside the view"),
    (dict(row=16), "pixel outside the view"),
    (dict(exp2=1, mrd=101), WIDE_EXP2),
]


@pytest.mark.parametrize("change, message", REFUSALS, ids=[",".join(c) for c, _ in REFUSALS])
def test_validator_refusals_status_and_message(change, message):
    """The host-only call refuses what the launch refuses in a view, with the wide validator's text, and writes nothing."""
    lib = L.load()
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    f = dict(dict(range_r=1.0, range_i=1.0, exp2=-50, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16), **change)
    cv = L.mbk_deep_xview(*[f[k] for k in ("range_r", "range_i", "exp2", "width", "height", "col0", "row0", "ncols", "nrows")])
    n, x, e = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    vals = [C.c_double(-7.0) for _ in range(4)]
    st = lib.mbk_deep_xview_distance_host(orbit._h if "orbit" not in change else None, C.byref(cv) if "view" not in change else None,
                                          f.get("col", 3), f.get("row", 4), f.get("mrd", 50), C.byref(n), C.byref(x),
                                          C.byref(vals[0]), C.byref(vals[1]), C.byref(vals[2]), C.byref(e),
                                          C.byref(vals[3]) if "out" not in change else None)
    assert (st, DEV._error_text(lib)) == (L.MBK_ERR_INVALID, message)
    assert (n.value, x.value, e.value) == (-7, -7, -7) and all(v.value == -7.0 for v in vals)


def test_the_served_call_writes_every_output():
    lib = L.load()
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    view = WideDeepView(1.0, -50, 16, 16)
    out = DEV.wide_distance_host(orbit, view, [4 * 16 + 3], 50)
    st = WD.states(*orbit.wide_table(), *(a[[4 * 16 + 3]] for a in W.offsets(view)), -50, 50)
    _assert_twin_equals(out, st, view, "served")
    assert lib.mbk_abi_version() == 5
