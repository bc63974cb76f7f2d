"""Relief shading for extended-range deep views on the CPU (include/mbk.h, the section of that name): the numpy model of the
contract (tests/deep_wide_relief_model.py, what the GPU is held to bit for bit) against the two wide distance models whose state
it claims to share, the host twin mbk_deep_xview_normal_host -- compiled from the functions the kernels use -- against the
model, the model against the mathematics (the unit vector of z / d in mpmath from the exact pixel coordinate), against the
plain deep relief model wherever a plain view can name the spans, the magnitude bound, the render rule and the refusals.
No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import deep_model as D
import deep_relief_model as RL
import deep_wide_bla_model as BL
import deep_wide_distance_bla_model as XD
import deep_wide_distance_model as WD
import deep_wide_model as W
import deep_wide_relief_model as WR
import relief_model as RM
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, MbkError, Palette, WideDeepView, deep_normal_host, wide_normal_host
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import device as DEV
from distributedmandelbrot_amd.image import relief_resolve_host
from test_deep_wide import SAME, TRUTH_CASES, _sample
from test_deep_wide_distance import REFUSALS

IDS = [c[-1] for c in TRUTH_CASES]
RULES = [False, True]            # xbla
_CACHE = {}
_TRUTH = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _case(centre, rng, exp2, mrd, bits, key):
    """The case's sample (test_deep_wide._sample: orbit, view, 150 seeded picks of a 64 x 64 view), the full view's table and
    the model's states on the picks under both rules: computed once, shared, left unchanged."""
    orbit, view, pick, dr, di, count, mag = _sample(centre, rng, exp2, mrd, bits, key)
    if key not in _CACHE:
        table = WR.table_of(orbit, view)
        st = {False: WR.states(*orbit.wide_table(), dr, di, exp2, mrd), True: WR.states(*orbit.wide_table(), dr, di, exp2, mrd, table)}
        for s in st.values():
            for a in s.values():
                a.setflags(write=False)
        _CACHE[key] = (table, st)
    return (orbit, view, pick, dr, di, count, mag) + _CACHE[key]


def _picks(exp2):
    """Those of tests/test_deep_wide_distance.py: the first 100 of the sample, the first 40 at exp2 = -3000."""
    return 40 if exp2 == -3000 else 100


def _nu_candidates(st, reach=2):
    """nu for a ln and a log2 within `reach` ulps of numpy's on either side: [(2 reach + 1)^2, N]; the first row is numpy's."""
    def near(a, j):
        for _ in range(abs(j)):
            a = np.nextafter(a, np.inf if j > 0 else -np.inf)
        return a

    n, mag = st["n"], st["mag_esc"]
    order = sorted(range(-reach, reach + 1), key=abs)
    outs = []
    with np.errstate(all="ignore"):
        l = np.log(mag)
        for j in order:
            g = np.log2(0.5 * near(l, j))
            for k in order:
                outs.append(np.where(n > 0, n + 1.0 - near(g, k), 0.0))
    return np.stack(outs)


def _assert_nu_agrees(got, st, what):
    """`got` is the model's nu bit for bit wherever the implementation's logarithms are numpy's, and elsewhere what
    neighbouring logarithms give: the rule of deep_wide_distance_model.assert_states_agree.  Returns the share of the first."""
    cand = _nu_candidates(st)
    got = np.asarray(got, np.float64).ravel()
    assert not np.isnan(got).any(), what
    hit = (_bits(cand) == _bits(got)[None, :]).any(axis=0)
    assert hit.all(), (what, int((~hit).sum()), [(int(i), int(st["n"][i]), float(st["mag_esc"][i]), float(got[i]), float(cand[0, i]))
                                                 for i in np.flatnonzero(~hit)[:5]])
    return float((_bits(cand[0]) == _bits(got)).mean())


def _assert_twin_equals(host, st, what):
    for k in ("n", "extra", "e", "t", "steps"):
        assert np.array_equal(host[k], st[k]), (what, k, int((host[k] != st[k]).sum()))
    for k in ("zpr", "zpi", "Dr", "Di"):
        assert np.array_equal(_bits(host[k]), _bits(st[k])), (what, k)
    assert np.array_equal(_bits(host["normal"]), _bits(WR.normals(st))), what
    return _assert_nu_agrees(host["nu"], st, what)


# ---- the model's loop is that of the two distance models ---------------------------------------------------------------

@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_the_loop_is_that_of_the_two_distance_models(centre, rng, exp2, mrd, bits, key):
    orbit, view, pick, dr, di, count, mag, table, st = _case(centre, rng, exp2, mrd, bits, key)
    xst = XD.states(*orbit.wide_table(), dr, di, exp2, mrd, table)
    for xbla, want in ((False, WD.states(*orbit.wide_table(), dr, di, exp2, mrd)), (True, xst)):
        got = st[xbla]
        for k in ("n", "extra", "e"):
            assert np.array_equal(got[k], want[k]), (xbla, k)
        for k in ("Dr", "Di", "mag", "dmagD"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (xbla, k)
    assert np.array_equal(st[True]["steps"], xst["steps"])
    assert np.array_equal(st[False]["steps"], np.where(st[False]["n"] > 0, st[False]["n"], mrd - 1))
    # the escaping step's mag is the count models': what the smooth values of a count launch are made from
    assert np.array_equal(st[False]["n"], count) and np.array_equal(_bits(st[False]["mag_esc"]), _bits(mag))
    c, mg, _ = BL.counts(*orbit.wide_table(), dr, di, exp2, mrd, table)
    assert np.array_equal(st[True]["n"], c) and np.array_equal(_bits(st[True]["mag_esc"]), _bits(mg))
    for xbla in RULES:
        s = st[xbla]
        esc = s["n"] > 0
        assert (s["mag_esc"][esc] >= 4.0).all() and (s["mag"][esc] >= s["mag_esc"][esc]).all() and not s["mag_esc"][~esc].any()


# ---- host twin == model ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xbla", RULES)
@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_host_twin_equals_the_model(centre, rng, exp2, mrd, bits, key, xbla):
    orbit, view, pick, dr, di, _, _, table, st = _case(centre, rng, exp2, mrd, bits, key)
    st = st[xbla]
    host = wide_normal_host(orbit, view, pick, mrd, xbla=xbla)
    share = _assert_twin_equals(host, st, (key, xbla))
    # rel of the same final state: the distance twins' against this model's states
    dist = DEV.wide_distance_xbla_host(orbit, view, pick, mrd) if xbla else DEV.wide_distance_host(orbit, view, pick, mrd)
    ln_share = WD.assert_states_agree(dist["rel"], st, view.range_r, view.exp2, (key, xbla))
    esc = st["n"] > 0
    print(f"{key} xbla={xbla}: {int(esc.sum())} of {pick.size} escaped, t {int(st['t'][esc].min())}..{int(st['t'][esc].max())}, "
          f"e {int(st['e'][esc].min())}..{int(st['e'][esc].max())}, host nu == numpy's on {share:.3f}, rel on {ln_share:.3f}")
    assert esc.sum() >= 0.8 * pick.size


@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=IDS)
def test_no_escaped_pick_is_flat_and_m_keeps_its_bound(centre, rng, exp2, mrd, bits, key):
    """(0, 0) and nu == 0 exactly where n == 0; m = |z conj(D)|^2 of an escaped pick lies in (2^-68, 2^5) (include/mbk.h)."""
    st = _case(centre, rng, exp2, mrd, bits, key)[8]
    for xbla in RULES:
        s = st[xbla]
        nrm, nu = WR.normals(s), WR.nu(s)
        esc = s["n"] > 0
        assert not np.isnan(nrm).any()
        assert np.array_equal((nrm != 0.0).any(axis=1), esc) and np.array_equal(nu != 0.0, esc)
        assert (np.abs(np.hypot(nrm[esc, 0], nrm[esc, 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
        zr, zi, Dr, Di = (s[k][esc] for k in ("zpr", "zpi", "Dr", "Di"))
        wr, wi = zr * Dr + zi * Di, zi * Dr - zr * Di
        m = wr * wr + wi * wi
        assert (m > 2.0 ** -68).all() and (m < 2.0 ** 5).all(), (m.min(), m.max())
        assert (np.maximum(np.abs(zr), np.abs(zi)) < 2.0).all() and (s["t"][esc] <= 33).all()
        assert (np.maximum(np.abs(Dr), np.abs(Di)) >= 0.5).all() and (np.maximum(np.abs(Dr), np.abs(Di)) < 1.0).all()


# ---- model == truth -----------------------------------------------------------------------------------------------------

def _truth(case, i):
    """The unit vector of z / d of pick i in mpmath, its count and its run-on length: computed once for both rules."""
    centre, rng, exp2, mrd, bits, key = case
    if (key, i) not in _TRUTH:
        orbit, view, pick, dr, di, _, _, table, st = _case(*case)
        _TRUTH[(key, i)] = WR.hp_normal(centre, dr[i], di[i], exp2, max(int(st[False]["n"][i]), int(st[True]["n"][i])),
                                        orbit.precision_bits + 128)
    return _TRUTH[(key, i)]


def _errors(case, xbla):
    """(the escaped picks among the first _picks, those whose (count, run-on) are the truth's, their |normal - truth|)"""
    st = _case(*case)[8][xbla]
    picks = _picks(case[2])
    nrm = WR.normals(st)
    esc = np.flatnonzero(st["n"][:picks] > 0)
    same, errs = [], []
    for i in esc:
        n, extra, (tx, ty) = _truth(case, i)
        if (n, extra) == (st["n"][i], st["extra"][i]):
            same.append(i)
            errs.append(math.hypot(nrm[i, 0] - tx, nrm[i, 1] - ty))
    return esc, np.array(same, np.int64), np.array(errs)


def _bound(xbla):
    return WR.XBLA_NORMAL_ERR if xbla else WR.WIDE_NORMAL_ERR


@pytest.mark.parametrize("xbla", RULES)
@pytest.mark.parametrize("case", TRUTH_CASES, ids=IDS)
def test_model_against_truth(case, xbla):
    """The figures this test prints are those of deep_wide_relief_model.MEASURED_NORMAL.  A pick whose (count, run-on) differs
    from the truth's is left out: at most 1 % of the escaped picks of a case, and none under the plain step."""
    key = case[-1]
    esc, same, errs = _errors(case, xbla)
    worst = errs.max()
    print(f"{key} xbla={xbla}: {esc.size} of {_picks(case[2])} escaped, {same.size} agree in (count, run-on), "
          f"worst |normal - truth| {worst:.3e} (recorded {WR.MEASURED_NORMAL[key][int(xbla)]:.1e})")
    assert esc.size >= 0.8 * _picks(case[2]), esc.size
    assert same.size >= 0.99 * esc.size, (same.size, esc.size)
    if not xbla:
        assert same.size == esc.size
    assert worst <= _bound(xbla), (worst, _bound(xbla))


def test_the_tolerance_follows_the_rule():
    """The worst measured, one digit rounded up, times 4; and never wider than 1e-4."""
    assert set(WR.MEASURED_NORMAL) == set(IDS)
    for xbla in RULES:
        worst = max(v[int(xbla)] for v in WR.MEASURED_NORMAL.values())
        digit = 10.0 ** math.floor(math.log10(worst))
        assert math.isclose(_bound(xbla), 4 * math.ceil(worst / digit - 1e-9) * digit, rel_tol=1e-12)
        assert _bound(xbla) <= 1e-4


@pytest.mark.parametrize("xbla", RULES)
@pytest.mark.parametrize("case", [c for c in TRUTH_CASES if c[-1] in ("mis-3000", "1e-400")], ids=["mis-3000", "1e-400"])
def test_cases_that_leave_binary64(case, xbla):
    """A nonzero share of the escaped picks end with e > 1024 -- a derivative binary64 cannot hold -- or pass a step whose z has
    t < -1022: their normals are unit vectors and meet the truth bound like any other.

    Measured: on "mis-3000" every escaped pick ends with e in 3022 .. 3042.  On "1e-400" NO pick meets either condition under
    either rule (90 escaped picks: e <= 49, t >= -4): the view spans 4 around c = 1e-400, so every pixel's own z = Z_m + dz is
    of order dc.  What binary64 cannot hold there is the reference orbit: every Z_m, m >= 1, has an exponent near -1328 and
    would be 0 in a binary64 table, and each step adds such an entry into z.  So on that case the share asserted is that of
    the picks whose steps formed z on an entry with exponent below -1022 (xmin of the model), which is all of them."""
    st = _case(*case)[8][xbla]
    esc, same, errs = _errors(case, xbla)
    out = (st["e"] > 1024) | (st["tmin"] < -1022)
    print(f"{case[-1]} xbla={xbla}: {int(out[esc].sum())} of {esc.size} escaped picks end with e > 1024 or pass t < -1022 "
          f"(e up to {int(st['e'][esc].max())}, t down to {int(st['tmin'][esc].min())}, orbit exponents down to {int(st['xmin'][esc].min())})")
    if case[-1] == "1e-400":
        out = out | (st["xmin"] < -1022)
    share = out[esc].mean()
    assert share > 0.0
    nrm = WR.normals(st)
    w = esc[out[esc]]
    assert (np.abs(np.hypot(nrm[w, 0], nrm[w, 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
    held = out[same]
    assert held.any() and (errs[held] <= _bound(xbla)).all()


# ---- a wide view of plain spans stores what the plain view stores ------------------------------------------------------

@pytest.mark.parametrize("centre, span_r, span_i, mrd, M, escaped", SAME, ids=[c[0][0][:12] + "@%g" % c[1] for c in SAME])
def test_wide_normals_equal_the_plain_deep_normals(centre, span_r, span_i, mrd, M, escaped):
    """Scaling by a power of two is exact and no operand of these plain runs is subnormal: on the whole 64 x 64 view, plain
    step, the wide model's normals are deep_relief_model's bit for bit -- no case of the seven is dropped -- and so is nu."""
    span_i = span_i or span_r
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i))
    assert (orbit.length, orbit.escaped) == (M, escaped)
    pn, pc, pnu, _, pst = RL.model(orbit, DeepView(span_r, 64, 64, span_i), mrd)
    rr, ri, exp2 = W.as_wide(span_r, span_i)
    wn, wc, wnu, _, wst = WR.model(orbit, WideDeepView(rr, exp2, 64, 64, ri), mrd)
    assert np.array_equal(wc, pc) and np.array_equal(wst["extra"], pst["extra"])
    assert np.array_equal(_bits(wn), _bits(pn)), int((_bits(wn) != _bits(pn)).any(axis=2).sum())
    assert np.array_equal(_bits(wnu), _bits(pnu))
    esc = pst["n"] > 0
    for a, b in (("zpr", "zpr"), ("zpi", "zpi")):      # (zr, zi) 2^t is the plain zp
        assert np.array_equal(np.ldexp(wst[a][esc], wst["t"][esc].astype(np.int32)), pst[b][esc]), a


# ---- edges -------------------------------------------------------------------------------------------------------------

def test_m_equals_one():
    """Centre -2: the orbit escapes at M = 1, there is no table, every step rebases: the host twin equals the model under both
    flags, and both flags agree."""
    mrd, exp2 = 400, -1100
    view = WideDeepView(1.0, exp2, 24, 20)
    orbit = DeepOrbit("-2", "0", mrd, min_span_exp2=view.min_span_exp2)
    assert orbit.length == 1 and WR.table_of(orbit, view) == []
    every = np.arange(24 * 20)
    st = {xbla: WR.model(orbit, view, mrd, xbla=xbla)[4] for xbla in RULES}
    host = {xbla: wide_normal_host(orbit, view, every, mrd, xbla=xbla) for xbla in RULES}
    for xbla in RULES:
        _assert_twin_equals(host[xbla], st[xbla], ("M == 1", xbla))
    for k in host[False]:
        assert host[False][k].tobytes() == host[True][k].tobytes(), k
    assert (st[False]["n"] > 0).sum() > every.size // 2


def test_windows_do_not_change_the_table():
    """The host twin of a windowed xbla view reads the full view's table: the same states on the same pixels."""
    mrd = 3000
    view = WideDeepView(1.0, -1100, 24, 20)
    orbit = DeepOrbit("0", "1", mrd, min_span_exp2=view.min_span_exp2)
    pix = np.array([5 * 24 + 3, 9 * 24 + 11, 15 * 24 + 15])
    whole = wide_normal_host(orbit, view, pix, mrd, xbla=True)
    part = wide_normal_host(orbit, view, pix, mrd, xbla=True, window=(3, 5, 13, 11))
    for k in whole:
        assert whole[k].tobytes() == part[k].tobytes(), k
    assert (whole["steps"] < whole["n"]).all() and (whole["n"] > 0).all()
    st = WR.model(orbit, view, mrd, window=(3, 5, 13, 11), xbla=True)[4]
    sub = np.array([0 * 13 + 0, 4 * 13 + 8, 10 * 13 + 12])
    _assert_twin_equals(part, {k: v[sub] for k, v in st.items()}, "window")


@pytest.mark.parametrize("xbla", RULES)
def test_shallow_mrd(xbla):
    view = WideDeepView(1.0, -1100, 8, 8)
    orbit = DeepOrbit("0", "1", 100, min_span_exp2=view.min_span_exp2)
    for mrd in (0, 1, 2):
        nrm, n, nu, rel, st = WR.model(orbit, view, mrd, xbla=xbla)
        host = wide_normal_host(orbit, view, np.arange(64), mrd, xbla=xbla)
        for a in (nrm, n, nu, rel, st["extra"], host["n"], host["extra"], host["normal"], host["nu"]):
            assert not a.any(), mrd
        assert np.array_equal(host["steps"], st["steps"]) and (st["steps"] == max(mrd - 1, 0)).all()


# ---- the render rule ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("xbla", RULES)
@pytest.mark.parametrize("s", [1, 2])
def test_render_rule_on_model_samples(s, xbla):
    """mbk_relief_resolve_host of the model's own samples of a wide view equals the numpy render rule."""
    w, h, mrd = 20, 12, 887          # (the counts of this view lie in 881 .. 916: about a tenth of the samples never escape)
    view = WideDeepView(1.0, -1100, w * s, h * s)
    orbit = DeepOrbit("0", "1", mrd, min_span_exp2=view.min_span_exp2)
    normals, counts, nu, _, _ = WR.model(orbit, view, mrd, xbla=xbla)
    assert (counts > 0).any() and (counts == 0).any() and len(np.unique(counts)) > 5
    rng = np.random.default_rng(41)
    pal = Palette(rng.integers(0, 256, size=(41, 4), dtype=np.uint8), inside=(3, 100, 250, 90), scale=1.7, offset=0.3)
    for light, height in (((math.cos(0.6), math.sin(0.6)), 1.25), ((0.0, 0.0), 2.0 ** 10), ((-1.0, 1.0), 0.0)):
        got = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=normals, light=light, height=height)
        want = RM.render(pal.entries, pal.inside, pal.scale, pal.offset, light[0], light[1], height, s, counts, nu, normals)
        assert np.array_equal(got, want), (s, xbla, light)


# ---- symbols, signatures, refusals -------------------------------------------------------------------------------------

NAMES = ("mbk_deep_xview_launch_normal", "mbk_deep_xview_compute_normal", "mbk_deep_xview_relief_render_launch",
         "mbk_deep_xview_relief_render_compute", "mbk_deep_xview_normal_host")


def test_signatures_and_symbols():
    lib = L.load()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.mbk_abi_version() == 5
    # the deep calls' signatures with the wide view's struct; the host twin has zp's exponent as one more output
    for name in NAMES[:4]:
        deep = L.SIGNATURES[name.replace("xview", "view")]
        assert L.SIGNATURES[name] == (deep[0], deep[1][:2] + [C.POINTER(L.mbk_deep_xview)] + deep[1][3:]), name
    deep = L.SIGNATURES["mbk_deep_normal_host"][1]
    assert L.SIGNATURES[NAMES[4]] == (C.c_int, deep[:1] + [C.POINTER(L.mbk_deep_xview)] + deep[2:10] + [C.POINTER(C.c_int32)] + deep[10:])
    assert lib.mbk_deep_xview_launch_normal(None, None, None, 10, 0, None, None, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_compute_normal(None, None, None, 10, 0, None, None, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_relief_render_launch(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_relief_render_compute(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
    for name in ("compute_wide_view_normals", "launch_wide_view_normals", "render_wide_view_relief", "launch_render_wide_view_relief"):
        assert callable(getattr(MandelbrotDevice, name))
    import distributedmandelbrot_amd as pkg
    assert "wide_normal_host" in pkg.__all__ and pkg.wide_normal_host is DEV.wide_normal_host


def _host_call(lib, orbit, cv, col=3, row=4, mrd=50, flags=0, null=None):
    """mbk_deep_xview_normal_host into sentinel outputs: (status, message, the outputs); null: the output to pass as NULL"""
    ints = {k: C.c_int32(-7) for k in ("count", "extra", "t", "e")}
    dbl = {k: C.c_double(-7.0) for k in ("zr", "zi", "Dr", "Di", "nu")}
    nrm = (C.c_double * 2)(-7.0, -7.0)
    steps = C.c_uint64(7)
    args = [("count", ints["count"]), ("extra", ints["extra"]), ("zr", dbl["zr"]), ("zi", dbl["zi"]), ("t", ints["t"]), ("Dr", dbl["Dr"]),
            ("Di", dbl["Di"]), ("e", ints["e"]), ("normal", nrm), ("nu", dbl["nu"]), ("steps", steps)]
    ptrs = [None if k == null else (v if k == "normal" else C.byref(v)) for k, v in args]
    st = lib.mbk_deep_xview_normal_host(orbit, cv, col, row, mrd, flags, *ptrs)
    vals = [v.value for v in ints.values()] + [v.value for v in dbl.values()] + list(nrm) + [steps.value]
    return st, DEV._error_text(lib) if st != L.MBK_OK else "", vals


UNTOUCHED = [-7] * 4 + [-7.0] * 5 + [-7.0, -7.0] + [7]
NO_WIDE_BLA = "MBK_DEEP_BLA is not implemented for extended-range deep views"
OTHER_FLAGS = "extended-range deep normals take MBK_DEEP_XBLA only (no kernel selection, no fp32)"


@pytest.mark.parametrize("flags", [0, L.MBK_DEEP_XBLA], ids=["plain", "xbla"])
@pytest.mark.parametrize("change, message", REFUSALS, ids=[",".join(c) for c, _ in REFUSALS])
def test_validator_refusals_status_and_message(change, message, flags):
    """The host-only call refuses what the launch refuses in a view, with the wide validator's text, and writes nothing."""
    lib = L.load()
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    f = dict(dict(range_r=1.0, range_i=1.0, exp2=-50, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16), **change)
    cv = L.mbk_deep_xview(*[f[k] for k in ("range_r", "range_i", "exp2", "width", "height", "col0", "row0", "ncols", "nrows")])
    st, text, vals = _host_call(lib, orbit._h if "orbit" not in change else None, C.byref(cv) if "view" not in change else None,
                                f.get("col", 3), f.get("row", 4), f.get("mrd", 50), flags, null="nu" if "out" in change else None)
    assert (st, text) == (L.MBK_ERR_INVALID, message)
    assert vals == UNTOUCHED


def test_flag_and_pointer_refusals_of_the_host_call():
    lib = L.load()
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    cv = L.mbk_deep_xview(1.0, 1.0, -50, 16, 16, 0, 0, 16, 16)
    for flags in (L.MBK_DEEP_BLA, L.MBK_DEEP_BLA | L.MBK_DEEP_XBLA, L.MBK_DEEP_BLA | L.KERNELS["group"]):
        assert _host_call(lib, orbit._h, C.byref(cv), flags=flags) == (L.MBK_ERR_INVALID, NO_WIDE_BLA, UNTOUCHED), flags
    for flags in (L.KERNELS["group"], L.KERNELS["scan"] | L.MBK_DEEP_XBLA, L.MBK_PRECISION_F32, L.MBK_WANT_COUNTS, L.MBK_WANT_BYTES, 0x80000000):
        assert _host_call(lib, orbit._h, C.byref(cv), flags=flags) == (L.MBK_ERR_INVALID, OTHER_FLAGS, UNTOUCHED), flags
    for null in ("count", "extra", "zr", "zi", "t", "Dr", "Di", "e", "normal", "nu", "steps"):
        assert _host_call(lib, orbit._h, C.byref(cv), null=null) == (L.MBK_ERR_INVALID, "NULL argument", UNTOUCHED), null
    # the served call writes every output, under both flags
    for flags in (0, L.MBK_DEEP_XBLA):
        st, _, vals = _host_call(lib, orbit._h, C.byref(cv), flags=flags)
        assert st == L.MBK_OK and all(a != b for a, b in zip(vals[2:-1], UNTOUCHED[2:-1])) and vals[0] >= 0 and vals[1] >= 0, vals
    view = WideDeepView(1.0, -50, 16, 16)
    for xbla in RULES:
        got = wide_normal_host(orbit, view, [4 * 16 + 3], 50, xbla=xbla)
        st = WR.states(*orbit.wide_table(), *(a[[4 * 16 + 3]] for a in W.offsets(view)), -50, 50, WR.table_of(orbit, view) if xbla else ())
        _assert_twin_equals(got, st, "served")


def test_each_family_names_the_other():
    """A DeepView to each new Python call raises ValueError naming the deep call; the deep family keeps refusing a WideDeepView
    with its MbkError."""
    orbit = DeepOrbit("0", "1", 100, min_span=1e-20)
    deep, wide = DeepView(1e-20, 8, 8), WideDeepView(1.0, -1100, 8, 8)
    pal = Palette(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="takes a WideDeepView.*deep_normal_host"):
        wide_normal_host(orbit, deep, [0], 50)
    with pytest.raises(ValueError, match="takes a WideDeepView.*compute_deep_view_normals"):
        MandelbrotDevice.compute_wide_view_normals(None, orbit, deep, 50)
    with pytest.raises(ValueError, match="takes a WideDeepView.*launch_deep_view_normals"):
        MandelbrotDevice.launch_wide_view_normals(None, orbit, deep, 50, d_normals=8)
    with pytest.raises(ValueError, match="takes a WideDeepView.*render_deep_view_relief"):
        MandelbrotDevice.render_wide_view_relief(None, orbit, deep, 50, palette=pal)
    with pytest.raises(ValueError, match="takes a WideDeepView.*launch_render_deep_view_relief"):
        MandelbrotDevice.launch_render_wide_view_relief(None, orbit, deep, 50, palette=pal, d_rgba=8)
    with pytest.raises(MbkError, match="DeepView only.*2\\^-960.*compute_wide_view_normals"):
        deep_normal_host(orbit, wide, [0], 50)
