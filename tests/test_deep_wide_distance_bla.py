"""Distance estimates for extended-range deep views with bilinear approximation on the CPU (include/mbk.h, the section of that
name): the host twins against the numpy model (tests/deep_wide_distance_bla_model.py) bit for bit, the no-skip identity with
the full-step wide distance, the model against d' = 2 z d + 1 in mpmath at P + 128 bits, the skip on synthetic operands,
Koebe's bound, signatures and refusals.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import deep_wide_bla_model as BL
import deep_wide_distance_bla_model as XD
import deep_wide_distance_model as WD
import deep_wide_model as W
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import device as DEV
from test_deep_wide import TRUTH_CASES, _sample

IDS = [c[-1] for c in TRUTH_CASES]
_STATES = {}


def _states(centre, rng, exp2, mrd, bits, key):
    """The case's sample (test_deep_wide._sample: orbit, view, 150 seeded picks) and the model's states on it, computed once."""
    orbit, view, pick, dr, di, count, _ = _sample(centre, rng, exp2, mrd, bits, key)
    if key not in _STATES:
        table = XD.table_of(orbit, view)
        st = XD.states(*orbit.wide_table(), dr, di, exp2, mrd, table)
        for a in st.values():
            a.setflags(write=False)
        xc, _, xs = BL.counts(*orbit.wide_table(), dr, di, exp2, mrd, table)
        assert np.array_equal(st["n"], xc) and np.array_equal(st["steps"], xs)     # the count and the steps are XBLA's
        _STATES[key] = st
    return orbit, view, pick, dr, di, _STATES[key]


def _assert_twin_equals(host, st, view, what):
    for k in ("n", "extra", "e"):
        assert np.array_equal(host[k], st[k]), (what, k, int((host[k] != st[k]).sum()))
    for k in ("mag", "Dr", "Di", "dmagD"):
        assert np.array_equal(host[k].view(np.uint64), st[k].view(np.uint64)), (what, k)
    return XD.assert_states_agree(host["rel"], st, view.range_r, view.exp2, what)


# ---- host twin == model ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_host_twin_equals_the_model(centre, rng, exp2, mrd, bits, key):
    orbit, view, pick, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    host = DEV.wide_distance_xbla_host(orbit, view, pick, mrd)
    share = _assert_twin_equals(host, st, view, key)
    assert np.array_equal(host["steps"], st["steps"])
    count, _, steps = DEV.deep_xbla_count_host(orbit, view, pick, mrd)
    assert np.array_equal(host["n"], count) and np.array_equal(host["steps"], steps)
    esc = st["n"] > 0
    ref = np.where(esc, st["n"], mrd - 1).sum()
    print(f"{key}: {int(esc.sum())} of {pick.size} escaped, steps executed / reference iterations {st['steps'].sum() / ref:.4f}, "
          f"e {int(st['e'][esc].min())}..{int(st['e'][esc].max())}, run-on {int(st['extra'][esc].min())}..{int(st['extra'][esc].max())}, "
          f"host ln == numpy ln on {share:.3f}")
    assert (st["mag"][esc] >= 4.0).all() and not st["mag"][~esc].any()
    assert ((st["mag"][esc] >= WD.RADIUS2) | (st["extra"][esc] == WD.RUN_ON)).all()
    if key != "1e-400":
        assert (st["first_skip"] > 0).mean() > 0.9 and st["steps"].sum() < 0.5 * ref     # these cases do skip


def _seeded_operand(rs):
    a, b = (float(v) for v in rs.uniform(-1, 1, 2))
    if rs.rand() < 0.5:
        a = math.copysign(rs.uniform(0.5, 1), a)
    else:
        b = math.copysign(rs.uniform(0.5, 1), b)
    return a, b


def _both_skips(Ar, Ai, ae, Br, Bi, be, Dr, Di, e):
    host = DEV.wide_distance_xbla_skip_host(Ar, Ai, ae, Br, Bi, be, Dr, Di, e)
    m = XD.skip(*(np.array([v]) for v in (Ar, Ai, ae, Br, Bi, be, Dr, Di, e)))
    model = (float(m[0][0]), float(m[1][0]), int(m[2][0]))
    assert [np.float64(v).view(np.uint64) for v in host[:2]] == [np.float64(v).view(np.uint64) for v in model[:2]], (host, model)
    assert host == model, (host, model, (Ar, Ai, ae, Br, Bi, be, Dr, Di, e))
    return host


def test_skip_on_synthetic_operands():
    # a zero D: d' = B, normalised
    assert _both_skips(0.75, -0.5, 40, 0.5, 0.25, -7, 0.0, 0.0, W.EZ) == (0.5, 0.25, -7)
    # a zero B: d' = A d
    Dr, Di, e = _both_skips(0.5, 0.0, 10, 0.0, 0.0, W.EZ, 0.5, 0.5, 3)
    assert (Dr, Di, e) == (0.5, 0.5, 12)
    # both zero
    assert _both_skips(0.75, -0.5, 40, 0.0, 0.0, W.EZ, 0.0, 0.0, W.EZ) == (0.0, 0.0, W.EZ)
    # exponents 1300 binades apart: the smaller addend is dropped, in either direction
    assert _both_skips(0.5, 0.0, 1300, 0.75, 0.25, 0, 0.5, 0.0, 2) == (0.5, 0.0, 1301)
    assert _both_skips(0.5, 0.0, -1300, 0.75, 0.25, 0, 0.5, 0.0, 0) == (0.75, 0.25, 0)
    # e may decrease, and is not floored at 0
    assert _both_skips(0.5, 0.0, -600, 0.5, 0.0, -700, 0.5, 0.0, 30)[2] == -571
    # A d cancels B exactly
    assert _both_skips(-1.0, 0.0, 0, 0.5, 0.0, 0, 0.5, 0.0, 0) == (0.0, 0.0, W.EZ)
    # e at the cap stays there
    assert _both_skips(0.9, 0.1, 5, 0.5, 0.0, 0, 0.6, 0.9, 1 << 30)[2] == 1 << 30
    rs = np.random.RandomState(11)
    for _ in range(400):
        Ar, Ai = _seeded_operand(rs)
        Br, Bi = _seeded_operand(rs)
        Dr, Di = _seeded_operand(rs)
        e = int(rs.randint(-1500, 1500))
        ae = int(rs.randint(-3000, 3000))
        be = ae + e + int(rs.choice([0, int(rs.randint(-60, 60)), int(rs.randint(1000, 1300)), -int(rs.randint(1000, 1300)),
                                     1300, -1300, int(rs.randint(-4000, 4000))]))
        _both_skips(Ar, Ai, ae, Br, Bi, be, Dr, Di, e)


# ---- no skip -----------------------------------------------------------------------------------------------------------

def test_no_level_is_taken_at_1e_400_and_every_state_is_the_wide_distance():
    centre, rng, exp2, mrd, bits, key = TRUTH_CASES[-1]
    assert key == "1e-400"
    orbit, view, pick, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    assert not st["first_skip"].any()
    plain = DEV.wide_distance_host(orbit, view, pick, mrd)
    host = DEV.wide_distance_xbla_host(orbit, view, pick, mrd)
    for k in ("n", "extra", "e", "mag", "Dr", "Di", "dmagD", "rel"):
        assert np.array_equal(host[k], plain[k]) and host[k].tobytes() == plain[k].tobytes(), k
    full = WD.states(*orbit.wide_table(), dr, di, exp2, mrd)
    for k in ("n", "extra", "e", "mag", "Dr", "Di", "dmagD"):
        assert st[k].tobytes() == full[k].tobytes(), k
    assert np.array_equal(host["steps"], np.where(host["n"] > 0, host["n"], mrd - 1))


def test_m_equals_one_equals_the_wide_distance():
    """Centre -2: the orbit escapes at M = 1, there is no table, and every step rebases."""
    mrd, exp2 = 400, -1100
    view = WideDeepView(1.0, exp2, 24, 20)
    orbit = DeepOrbit("-2", "0", mrd, min_span_exp2=view.min_span_exp2)
    assert orbit.length == 1 and XD.table_of(orbit, view) == []
    rel, n, st = XD.model(orbit, view, mrd)
    frel, fn, fst = WD.model(orbit, view, mrd)
    for k in ("n", "extra", "e", "mag", "Dr", "Di", "dmagD"):
        assert st[k].tobytes() == fst[k].tobytes(), k
    assert rel.tobytes() == frel.tobytes() and (n > 0).sum() > n.size // 2
    every = np.arange(n.size)
    host, plain = DEV.wide_distance_xbla_host(orbit, view, every, mrd), DEV.wide_distance_host(orbit, view, every, mrd)
    _assert_twin_equals(host, st, view, "M == 1")
    for k in ("n", "extra", "e", "mag", "Dr", "Di", "rel"):
        assert host[k].tobytes() == plain[k].tobytes(), k


@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES[:4], ids=IDS[:4])
def test_up_to_its_first_skip_a_pixel_is_the_wide_distance_models(centre, rng, exp2, mrd, bits, key):
    """Cut the run off just before each pick's first skip (mrd = its step index: steps 1 .. i - 1 run, and a level that would
    reach past mrd is not taken -- level 0 is, so the cut is at the first index whose step ran plain): both models hold the
    same derivative there."""
    orbit, view, pick, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    table = XD.table_of(orbit, view)
    firsts = st["first_skip"][:24]
    assert (firsts > 0).all()
    for j, cut in enumerate(firsts):
        a = XD.states(*orbit.wide_table(), dr[j:j + 1], di[j:j + 1], exp2, int(cut), table)
        b = WD.states(*orbit.wide_table(), dr[j:j + 1], di[j:j + 1], exp2, int(cut))
        assert not a["first_skip"].any() and a["steps"][0] == max(int(cut) - 1, 0)
        for k in ("n", "extra", "e", "mag", "Dr", "Di"):
            assert a[k].tobytes() == b[k].tobytes(), (j, int(cut), k)


# ---- model == truth -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_model_against_truth(centre, rng, exp2, mrd, bits, key):
    """The picks of tests/test_deep_wide_distance.py: the first 100 of the sample's 150, the first 40 at exp2 = -3000.
    (count, run-on) agree on at least 99 % of the escaped picks -- a condition on the inputs: the wide XBLA model equals the
    truth's count on every sampled pixel of these cases."""
    orbit, view, pick, dr, di, st = _states(centre, rng, exp2, mrd, bits, key)
    picks = 40 if exp2 == -3000 else 100
    rel = WD.value(st["mag"], st["dmagD"], st["e"], rng, exp2, st["n"])[:picks]
    n = st["n"][:picks]
    esc = np.flatnonzero(n > 0)
    errs, agree = [], 0
    for i in esc:
        ok, truth = XD.hp_sample(centre, dr[i], di[i], rng, exp2, n[i], st["extra"][i], orbit.precision_bits + 128)
        if ok:
            agree += 1
            errs.append(abs(rel[i] - truth) / truth)
    worst = max(errs)
    print(f"{key}: {esc.size} of {picks} escaped, {agree} agree in (count, run-on), counts {n[esc].min()}..{n[esc].max()}, "
          f"e {int(st['e'][:picks][esc].min())}..{int(st['e'][:picks][esc].max())}, worst relative error of rel {worst:.3e}")
    assert agree >= 0.99 * esc.size, (agree, esc.size)
    assert np.isfinite(rel[esc]).all() and (rel[esc] > 0).all()
    assert worst <= XD.XBLA_DERIVATIVE_REL, worst


def test_the_tolerance_follows_the_rule():
    """The worst measured, one digit rounded up, times 4; and never wider than 1e-4."""
    worst = max(XD.MEASURED_REL.values())
    digit = 10.0 ** math.floor(math.log10(worst))
    assert set(XD.MEASURED_REL) == set(IDS)
    assert math.isclose(XD.XBLA_DERIVATIVE_REL, 4 * math.ceil(worst / digit - 1e-9) * digit, rel_tol=1e-12)
    assert XD.XBLA_DERIVATIVE_REL <= 1e-4


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
    assert (ratio <= 1.0 + XD.XBLA_DERIVATIVE_REL).all() and ratio.max() > 0.01


def test_windows_do_not_change_dcmax():
    """The host twin of a windowed view reads the full view's table: the same states on the same pixels."""
    mrd = 3000
    view = WideDeepView(1.0, -1100, 24, 20)
    orbit = DeepOrbit("0", "1", mrd, min_span_exp2=view.min_span_exp2)
    pix = np.array([5 * 24 + 3, 9 * 24 + 11, 15 * 24 + 15])
    whole = DEV.wide_distance_xbla_host(orbit, view, pix, mrd)
    part = DEV.wide_distance_xbla_host(orbit, view, pix, mrd, window=(3, 5, 13, 11))
    for k in whole:
        assert whole[k].tobytes() == part[k].tobytes(), k
    assert (whole["steps"] < whole["n"]).all() and (whole["n"] > 0).all()
    rel, n, st = XD.model(orbit, view, mrd, window=(3, 5, 13, 11))
    sub = np.array([0 * 13 + 0, 4 * 13 + 8, 10 * 13 + 12])
    _assert_twin_equals(part, {k: v[sub] for k, v in st.items()}, view, "window")


def test_signatures_and_symbols():
    lib = L.load()
    names = ("mbk_deep_xview_launch_distance_xbla", "mbk_deep_xview_compute_distance_xbla", "mbk_deep_xview_distance_xbla_render_launch",
             "mbk_deep_xview_distance_xbla_render_compute", "mbk_deep_xview_distance_xbla_host", "mbk_deep_xdistance_skip_host")
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.mbk_abi_version() == 5
    for name in names[:2]:
        assert getattr(lib, name)(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
        assert L.SIGNATURES[name] == L.SIGNATURES[name.replace("_xbla", "")]
    for name in names[2:4]:
        assert getattr(lib, name)(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
        assert L.SIGNATURES[name] == L.SIGNATURES[name.replace("_xbla", "")]
    assert L.SIGNATURES[names[4]][1] == L.SIGNATURES["mbk_deep_xview_distance_host"][1] + [C.POINTER(C.c_uint64)]
    assert lib.mbk_deep_xdistance_skip_host(0.5, 0.5, 0, 0.5, 0.0, 0, None, None, None) == L.MBK_ERR_INVALID
    assert DEV._error_text(lib) == "NULL argument"
    for name in ("compute_wide_view_distance_xbla", "launch_wide_view_distance_xbla", "render_wide_view_distance_xbla",
                 "launch_render_wide_view_distance_xbla"):
        assert callable(getattr(MandelbrotDevice, name))
    assert callable(DEV.wide_distance_xbla_host) and callable(DEV.wide_distance_xbla_skip_host)


WIDE_RANGE = "extended-range deep view ranges must be finite and lie in [2^-64, 4]"
WIDE_EXP2 = "extended-range deep view exp2 must lie in [-8192, 0]"
# (what differs from a served call, the message); orbit mrd 100, view 16 x 16 of span 2^-50, pixel (3, 4), mrd 50
REFUSALS = [
    (dict(orbit=None), "orbit is NULL"),
    (dict(view=None), "view is NULL"),
    (dict(out=None), "NULL argument"),
    (dict(steps=None), "NULL argument"),
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
    n, x, e, s = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7), C.c_uint64(7)
    vals = [C.c_double(-7.0) for _ in range(4)]
    st = lib.mbk_deep_xview_distance_xbla_host(orbit._h if "orbit" not in change else None, C.byref(cv) if "view" not in change else None,
                                               f.get("col", 3), f.get("row", 4), f.get("mrd", 50), C.byref(n), C.byref(x),
                                               C.byref(vals[0]), C.byref(vals[1]), C.byref(vals[2]), C.byref(e),
                                               C.byref(vals[3]) if "out" not in change else None,
                                               C.byref(s) if "steps" not in change else None)
    assert (st, DEV._error_text(lib)) == (L.MBK_ERR_INVALID, message)
    assert (n.value, x.value, e.value, s.value) == (-7, -7, -7, 7) and all(v.value == -7.0 for v in vals)


def test_the_served_call_writes_every_output():
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    view = WideDeepView(1.0, -50, 16, 16)
    out = DEV.wide_distance_xbla_host(orbit, view, [4 * 16 + 3], 50)
    st = XD.states(*orbit.wide_table(), *(a[[4 * 16 + 3]] for a in W.offsets(view)), -50, 50, XD.table_of(orbit, view))
    _assert_twin_equals(out, st, view, "served")
    assert out["steps"][0] == st["steps"][0]
