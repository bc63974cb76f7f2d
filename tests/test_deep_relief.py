"""Relief shading for deep views on the CPU (include/mbk.h, "Relief shading for deep views"): the numpy model of the contract
(tests/deep_relief_model.py, what the GPU is held to bit for bit) against the two distance models whose state it claims to share,
the host twin mbk_deep_normal_host -- compiled from the functions the kernels use -- against the model on every bit, the model
against the mathematics (the unit vector of z / d in mpmath from the exact pixel coordinate), and the render rule.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import deep_bla_model as BL
import deep_distance_bla_model as DB
import deep_distance_model as DD
import deep_model as D
import deep_relief_model as RL
import relief_model as RM
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, WideDeepView, deep_normal_host
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import relief_resolve_host
from test_deep_distance import CASES, PICKS

RULES = [False, True]            # bla
_CACHE = {}
_TRUTH = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _case(name):
    """The seeded picks of a 64 x 64 view, as test_deep_distance._case makes them, and the model's states on them under both
    rules: computed once, shared, left unchanged."""
    if name not in _CACHE:
        centre, span, mrd = CASES[name]
        orbit = DeepOrbit(*centre, mrd, min_span=span)
        view = DeepView(span, 64, 64)
        dr, di = D.offsets(view)
        pick = np.random.RandomState(1).choice(dr.size, PICKS, replace=False)
        zr, zi = orbit.table()
        table = BL.build(zr, zi, BL.dcmax(view))
        st = {False: RL.states(zr, zi, dr[pick], di[pick], mrd), True: RL.states(zr, zi, dr[pick], di[pick], mrd, table)}
        _CACHE[name] = (orbit, view, pick, dr[pick], di[pick], table, st)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_loop_is_that_of_the_two_distance_models(name):
    centre, span, mrd = CASES[name]
    orbit, view, pick, dr, di, table, st = _case(name)
    zr, zi = orbit.table()
    for bla, want in ((False, DD.states(zr, zi, dr, di, mrd)), (True, DB.states(zr, zi, dr, di, mrd, table))):
        got = st[bla]
        for k in ("n", "extra", "e"):
            assert np.array_equal(got[k], want[k]), (bla, k)
        for k in ("Dr", "Di", "mag", "dmagD"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (bla, k)
    assert np.array_equal(st[True]["steps"], DB.states(zr, zi, dr, di, mrd, table)["steps"])
    assert np.array_equal(st[False]["steps"], np.where(st[False]["n"] > 0, st[False]["n"], mrd - 1))
    # the escaping step's mag is the count models': what the smooth values of a count launch are made from
    c, mg = D.model_counts(zr, zi, dr, di, mrd)
    assert np.array_equal(st[False]["n"], c) and np.array_equal(_bits(st[False]["mag_esc"]), _bits(mg))
    c, mg, _ = BL.counts(zr, zi, dr, di, mrd, table)
    assert np.array_equal(st[True]["n"], c) and np.array_equal(_bits(st[True]["mag_esc"]), _bits(mg))
    for bla in RULES:
        esc = st[bla]["n"] > 0
        assert (st[bla]["mag_esc"][esc] >= 4.0).all() and (st[bla]["mag"][esc] >= st[bla]["mag_esc"][esc]).all()
        assert not st[bla]["mag_esc"][~esc].any()


@pytest.mark.parametrize("bla", RULES)
@pytest.mark.parametrize("name", list(CASES))
def test_host_twin_equals_the_model_on_every_bit(name, bla):
    centre, span, mrd = CASES[name]
    orbit, view, pick, dr, di, table, st = _case(name)
    st = st[bla]
    got = deep_normal_host(orbit, view, pick, mrd, bla=bla)
    for k in ("n", "extra", "e", "steps"):
        assert np.array_equal(got[k], st[k]), k
    for k in ("zpr", "zpi", "Dr", "Di"):
        assert np.array_equal(_bits(got[k]), _bits(st[k])), k
    want = RL.normals(st)
    assert np.array_equal(_bits(got["normal"]), _bits(want))
    assert np.array_equal(_bits(got["nu"]), _bits(RL.nu(st)))            # numpy's logarithms are the host libm's
    esc = st["n"] > 0
    assert esc.sum() >= 0.9 * PICKS and not np.isnan(want).any()
    assert (np.abs(np.hypot(want[esc, 0], want[esc, 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all()      # none flat
    assert not want[~esc].any()


def test_e_drops_out():
    """At 1e-200 every escaped pixel ends with e >= 512: the normal is formed from D alone and is a unit vector all the same."""
    for bla in RULES:
        st = _case("i-1e-200")[6][bla]
        esc = st["n"] > 0
        assert (st["e"][esc] >= 512).all()
        nrm = RL.normals(st)
        assert (np.abs(np.hypot(nrm[esc, 0], nrm[esc, 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
        m = (st["zpr"] ** 2 + st["zpi"] ** 2) * st["dmagD"]
        assert (m[esc] < 2.0 ** 580).all() and (m[esc] > 0).all()


def _no_skip_cases():
    # those of tests/test_deep_distance_bla.py: an orbit of length 1 (no table), and a thin view whose offsets never pass
    # level 0's radius
    return {"M == 1": (("-2", "0"), 1e-10, None, 1000), "-0.75 span_i 4e-3": (("-0.75", "0"), 1e-25, 4e-3, 5000)}


@pytest.mark.parametrize("name", list(_no_skip_cases()))
def test_no_skip_identity(name):
    centre, span_r, span_i, mrd = _no_skip_cases()[name]
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i or span_r))
    assert (orbit.length == 1) == (name == "M == 1")
    view = DeepView(span_r, 64, 64, span_i)
    zr, zi = orbit.table()
    dr, di = D.offsets(view)
    pick = np.random.RandomState(2).choice(dr.size, 200, replace=False)
    table = BL.build(zr, zi, BL.dcmax(view))
    with_table = RL.states(zr, zi, dr[pick], di[pick], mrd, table)
    plain = RL.states(zr, zi, dr[pick], di[pick], mrd)
    assert np.array_equal(with_table["steps"], np.where(plain["n"] > 0, plain["n"], mrd - 1)) and (plain["n"] > 0).any()
    a, b = deep_normal_host(orbit, view, pick, mrd, bla=True), deep_normal_host(orbit, view, pick, mrd, bla=False)
    for k in ("n", "extra", "e", "steps"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], plain[k]) and np.array_equal(with_table[k], plain[k]), k
    for k in ("zpr", "zpi", "Dr", "Di", "normal", "nu"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(_bits(a["normal"]), _bits(RL.normals(plain))) and np.array_equal(_bits(a["nu"]), _bits(RL.nu(plain)))


def _truth(name, i):
    """The unit vector of z / d of pick i in mpmath, its count and its run-on length: computed once for both rules."""
    if (name, i) not in _TRUTH:
        centre, span, mrd = CASES[name]
        orbit, view, pick, dr, di, table, st = _case(name)
        _TRUTH[(name, i)] = RL.hp_normal(centre, dr[i], di[i], max(int(st[False]["n"][i]), int(st[True]["n"][i])),
                                         orbit.precision_bits + 128)
    return _TRUTH[(name, i)]


@pytest.mark.parametrize("bla", RULES)
@pytest.mark.parametrize("name", list(CASES))
def test_model_against_truth(name, bla):
    """The figures this test prints are those of deep_relief_model.MEASURED_NORMAL; the bound is the worst of the rule, one
    digit rounded up, times 4."""
    st = _case(name)[6][bla]
    nrm = RL.normals(st)
    esc = np.flatnonzero(st["n"] > 0)
    assert esc.size >= 0.9 * PICKS, esc.size
    errs = []
    for i in esc:
        n, extra, (tx, ty) = _truth(name, i)
        if (n, extra) == (st["n"][i], st["extra"][i]):
            errs.append(math.hypot(nrm[i, 0] - tx, nrm[i, 1] - ty))
    worst = max(errs)
    print(f"{name} bla={bla}: {esc.size} of {PICKS} escaped, {len(errs)} agree in (count, run-on), worst |normal - truth| {worst:.3e} "
          f"(recorded {RL.MEASURED_NORMAL[name][int(bla)]:.1e})")
    assert len(errs) >= 0.9 * esc.size, (len(errs), esc.size)               # at most 10 % left out
    bound = RL.DEEP_BLA_NORMAL_ERR if bla else RL.DEEP_NORMAL_ERR
    assert worst <= bound, (worst, bound)
    assert math.isclose(bound, _convention(max(v[int(bla)] for v in RL.MEASURED_NORMAL.values())), rel_tol=1e-12)


def _convention(worst):
    """One digit, rounded up, times 4."""
    exp = math.floor(math.log10(worst))
    return 4 * math.ceil(worst / 10.0 ** exp - 1e-9) * 10.0 ** exp


def _palette(n=41, scale=1.7, offset=0.3):
    rng = np.random.default_rng(n)
    return Palette(rng.integers(0, 256, size=(n, 4), dtype=np.uint8), inside=(3, 100, 250, 90), scale=scale, offset=offset)


@pytest.mark.parametrize("bla", RULES)
@pytest.mark.parametrize("s", [1, 2, 3])
def test_render_rule_on_model_samples(s, bla):
    """mbk_relief_resolve_host of the model's own samples of a deep view equals the numpy render rule."""
    centre, span, mrd = CASES["seahorse-1e-12"]
    orbit = _case("seahorse-1e-12")[0]
    w, h = 10, 7
    normals, counts, nu, _, _ = RL.model(orbit, DeepView(span, w * s, h * s), 600, bla=bla)
    assert (counts > 0).any() and len(np.unique(counts)) > 5
    pal = _palette()
    for light, height in (((math.cos(0.6), math.sin(0.6)), 1.25), ((0.0, 0.0), 2.0 ** 10), ((-1.0, 1.0), 0.0)):
        got = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=normals, light=light, height=height)
        want = RM.render(pal.entries, pal.inside, pal.scale, pal.offset, light[0], light[1], height, s, counts, nu, normals)
        assert np.array_equal(got, want), (s, bla, light)


def test_signatures_symbols_and_host_refusals():
    lib = L.load()
    names = ("mbk_deep_view_launch_normal", "mbk_deep_view_compute_normal", "mbk_deep_view_relief_render_launch",
             "mbk_deep_view_relief_render_compute", "mbk_deep_normal_host")
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mbk_abi_version() == 5
    assert lib.mbk_deep_view_launch_normal(None, None, None, 10, 0, None, None, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_compute_normal(None, None, None, 10, 0, None, None, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_relief_render_launch(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_relief_render_compute(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
    orbit = DeepOrbit("0", "1", 100, min_span=1e-20)
    view = DeepView(1e-20, 8, 8)
    for bla in RULES:
        with pytest.raises(MbkError):
            deep_normal_host(orbit, view, [64], 100, bla=bla)                 # a pixel outside the view
        with pytest.raises(MbkError):
            deep_normal_host(orbit, view, [0], 101, bla=bla)                  # mrd above the orbit's
        for mrd in (0, 1):
            got = deep_normal_host(orbit, view, np.arange(64), mrd, bla=bla)
            assert not got["n"].any() and not got["normal"].any() and not got["nu"].any() and not got["steps"].any()
    with pytest.raises(MbkError, match="DeepView only"):
        deep_normal_host(orbit, WideDeepView(1.0, -1100, 8, 8), [0], 100)
    # the C call: every flag but MBK_DEEP_BLA, a NULL output, ranges below 2^-960
    cv = L.mbk_deep_view(1e-20, 1e-20, 8, 8, 0, 0, 8, 8)
    n, x, e, s = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_uint64(7)
    d = [C.c_double(7.0) for _ in range(5)]
    nrm = (C.c_double * 2)(7.0, 7.0)

    def call(flags, view=cv, normal=nrm, orb=orbit._h):
        return lib.mbk_deep_normal_host(orb, C.byref(view), 0, 0, 50, flags, C.byref(n), C.byref(x), C.byref(d[0]), C.byref(d[1]),
                                        C.byref(d[2]), C.byref(d[3]), C.byref(e), normal, C.byref(d[4]), C.byref(s))

    for flags in (L.MBK_DEEP_XBLA, L.MBK_PRECISION_F32, L.MBK_WANT_COUNTS, L.KERNELS["group"], L.MBK_DEEP_BLA | 0x1, 0x80000000):
        assert call(flags) == L.MBK_ERR_INVALID, flags
    assert call(0, normal=None) == L.MBK_ERR_INVALID and call(0, orb=None) == L.MBK_ERR_INVALID
    assert call(0, view=L.mbk_deep_view(2.0 ** -1000, 2.0 ** -1000, 8, 8, 0, 0, 8, 8)) == L.MBK_ERR_INVALID
    assert (n.value, x.value, e.value, s.value) == (7, 7, 7, 7) and all(v.value == 7.0 for v in d) and tuple(nrm) == (7.0, 7.0)
    assert call(0) == call(L.MBK_DEEP_BLA) == L.MBK_OK and (n.value, x.value) == (0, 0) and tuple(nrm) == (0.0, 0.0)
