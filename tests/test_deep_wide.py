"""Extended-range deep views on the CPU (include/mbk.h, "Extended-range deep views"): the wide orbit table against a
Python-integer restatement, the host twin of the step against the numpy model (tests/deep_wide_model.py) bit for bit, the
model against the plain deep model wherever a plain view can name the spans, and against z = z^2 + c iterated directly in
fixed point at P + 128 fraction bits on spans of 2^-1100 and 2^-3000 and on a centre the binary64 table cannot hold."""
import ctypes as C
from decimal import Decimal, getcontext

import numpy as np
import pytest

import deep_model as D
import deep_wide_model as W
from test_deep_truth import CASES as PLAIN_CASES

from distributedmandelbrot_amd import DeepOrbit, DeepView, WideDeepView
from distributedmandelbrot_amd import _lib as L


def _misiurewicz() -> str:
    """The real root of c^3 + 2c^2 + 2c + 2 (the tip of the period-3 antenna's preperiodic point) to 1300 digits, by Newton."""
    old = getcontext().prec
    getcontext().prec = 1320
    try:
        c = Decimal("-1.5436890126920763615708559718")
        for _ in range(12):
            c = c - (((c + 2) * c + 2) * c + 2) / ((3 * c + 4) * c + 2)
        return str(c.quantize(Decimal(10) ** -1300))
    finally:
        getcontext().prec = old


MIS = (_misiurewicz(), "0")
TINY = ("1e-400", "0")

# (centre, range, exp2, mrd, precision_bits (None: the default for the span), id)
TRUTH_CASES = [
    (("0", "1"), 1.0, -1100, 3000, None, "i-1100"),
    (("0", "1"), 1.0, -3000, 6000, None, "i-3000"),
    (MIS, 1.0, -1100, 4000, None, "mis-1100"),
    (MIS, 1.0, -3000, 9000, None, "mis-3000"),
    (TINY, 4.0, 0, 300, 1408, "1e-400"),        # span 4 around a centre whose every Z_m is below 1e-308 at each return to 0
]


def _orbit(centre, view, mrd, bits):
    return DeepOrbit(*centre, mrd, precision_bits=bits) if bits else DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)


_cache = {}


def _sample(centre, rng, exp2, mrd, bits, key):
    """The case's orbit, 150 seeded pixels of its 64 x 64 view, and the model on them (computed once, shared)."""
    if key not in _cache:
        view = WideDeepView(rng, exp2, 64, 64)
        orbit = _orbit(centre, view, mrd, bits)
        dr, di = W.offsets(view)
        pick = np.random.RandomState(1).choice(dr.size, 150, replace=False)
        count, mag = W.model_counts(*orbit.wide_table(), dr[pick], di[pick], exp2, mrd)
        count.setflags(write=False)
        mag.setflags(write=False)
        _cache[key] = (orbit, view, pick, dr[pick], di[pick], count, mag)
    return _cache[key]


def _host(orbit, view, pick, mrd):
    lib = L.load()
    cv = L.mbk_deep_xview(view.range_r, view.range_i, view.exp2, view.width, view.height, 0, 0, view.width, view.height)
    count = np.empty(pick.size, np.int32)
    mag = np.empty(pick.size, np.float64)
    c, m = C.c_int32(), C.c_double()
    for j, k in enumerate(pick):
        assert lib.mbk_deep_xview_count_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), mrd,
                                             C.byref(c), C.byref(m)) == L.MBK_OK
        count[j], mag[j] = c.value, m.value
    return count, mag


# ---- the wide table -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centre, bits, mrd, M", [(("0", "1"), 192, 200, 200), (TINY, 1408, 300, 300), (("-2", "0"), 128, 50, 1)],
                         ids=["i", "1e-400", "-2"])
def test_wide_table_equals_the_integer_restatement(centre, bits, mrd, M):
    orbit = DeepOrbit(*centre, mrd, precision_bits=bits)
    assert orbit.length == M
    xr, xi, xe = orbit.wide_table()
    mr, mi, me = W.wide_table(centre[0], centre[1], bits, mrd)
    assert xe.dtype == np.int32 and np.array_equal(xe, me)
    assert np.array_equal(xr.view(np.uint64), mr.view(np.uint64)) and np.array_equal(xi.view(np.uint64), mi.view(np.uint64))
    assert (xr[0], xi[0], xe[0]) == (0.0, 0.0, W.EZ)
    big = np.maximum(np.abs(xr[1:]), np.abs(xi[1:]))
    assert ((big >= 0.5) & (big <= 1.0)).all()
    # X 2^xe is the binary64 table wherever that holds a normal number
    zr, zi = orbit.table()
    for x, z in ((xr, zr), (xi, zi)):
        normal = np.abs(z) >= 2.0 ** -1022
        assert np.array_equal(np.ldexp(x, xe)[normal].view(np.uint64), z[normal].view(np.uint64))
    if centre == TINY:
        # every entry lies near 2^-1328, where the binary64 table holds nothing
        assert (np.abs(xe[1:] + 1328) <= 2).all() and not zr.any() and not zi.any()
    if centre == ("0", "1"):
        assert normal.sum() > M // 2


def test_wide_table_capacity_is_checked():
    orbit = DeepOrbit("0", "1", 20, precision_bits=64)
    xr, xi, xe = np.full(20, 7.0), np.full(20, 7.0), np.full(20, 7, np.int32)
    assert L.load().mbk_deep_orbit_read_wide(orbit._h, xr.ctypes.data, xi.ctypes.data, xe.ctypes.data, 20) == L.MBK_ERR_INVALID
    assert (xr == 7.0).all() and (xe == 7).all()


# ---- host twin == model, model == truth ----------------------------------------------------------------------------

@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=[c[-1] for c in TRUTH_CASES])
def test_host_twin_equals_the_model(centre, rng, exp2, mrd, bits, key):
    orbit, view, pick, _, _, count, mag = _sample(centre, rng, exp2, mrd, bits, key)
    hc, hm = _host(orbit, view, pick, mrd)
    assert np.array_equal(hc, count), int((hc != count).sum())
    assert np.array_equal(hm.view(np.uint64), mag.view(np.uint64))
    assert ((mag >= 4.0) == (count > 0)).all()


@pytest.mark.parametrize("centre, rng, exp2, mrd, bits, key", TRUTH_CASES, ids=[c[-1] for c in TRUTH_CASES])
def test_model_equals_direct_iteration(centre, rng, exp2, mrd, bits, key):
    """>= 99 % of the sampled pixels equal the truth, at least 8 distinct counts in the truth: the caps of the plain contract.
    Measured: every pixel equal on all five cases."""
    orbit, view, pick, dr, di, count, _ = _sample(centre, rng, exp2, mrd, bits, key)
    truth = W.direct_counts(centre[0], centre[1], dr, di, exp2, mrd, orbit.precision_bits + 128)
    print(key, "equal", float((count == truth).mean()), "distinct", len(np.unique(truth)), "range", truth.min(), truth.max())
    assert len(np.unique(truth)) >= 8, np.unique(truth)
    assert (count == truth).mean() >= 0.99, (int((count != truth).sum()), np.unique(count), np.unique(truth))


def test_m_equals_one_host_twin_equals_the_model():
    """Centre -2: the orbit escapes at M = 1 and every step rebases.  Model only: the tip is a known limit of the truth."""
    mrd, exp2 = 400, -1100
    view = WideDeepView(1.0, exp2, 24, 20)
    orbit = DeepOrbit("-2", "0", mrd, min_span_exp2=view.min_span_exp2)
    assert orbit.length == 1 and orbit.escaped
    dr, di = W.offsets(view)
    count, mag = W.model_counts(*orbit.wide_table(), dr, di, exp2, mrd)
    hc, hm = _host(orbit, view, np.arange(dr.size), mrd)
    assert np.array_equal(hc, count) and np.array_equal(hm.view(np.uint64), mag.view(np.uint64))


# ---- a wide view of plain spans stores what the plain view stores --------------------------------------------------------

def _aspect_fits(span_r, span_i):
    return max(span_r, span_i) / min(span_r, span_i) <= 2.0 ** 64


SAME = [c for c in PLAIN_CASES if _aspect_fits(c[1], c[2] or c[1])]


def test_the_catalogue_keeps_most_of_its_cases():
    assert len(SAME) == 7 and len(PLAIN_CASES) == 9      # the two views with spans 2^75 and 2^86 apart cannot be named


@pytest.mark.parametrize("centre, span_r, span_i, mrd, M, escaped", SAME, ids=[c[0][0][:12] + "@%g" % c[1] for c in SAME])
def test_wide_model_equals_the_plain_model(centre, span_r, span_i, mrd, M, escaped):
    """Scaling by a power of two is exact, and no value of these plain runs is subnormal: counts and mag are equal bit for
    bit, on the whole 64 x 64 view; and the host twin equals both on a sample."""
    span_i = span_i or span_r
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i))
    assert (orbit.length, orbit.escaped) == (M, escaped)
    plain = DeepView(span_r, 64, 64, span_i)
    pc, pm = D.model_counts(*orbit.table(), *D.offsets(plain), mrd)
    rr, ri, exp2 = W.as_wide(span_r, span_i)
    assert 2.0 ** -64 <= min(rr, ri) and max(rr, ri) <= 4.0 and -8192 <= exp2 <= 0
    assert np.ldexp(rr, exp2) == span_r and np.ldexp(ri, exp2) == span_i
    view = WideDeepView(rr, exp2, 64, 64, ri)
    wc, wm = W.model_counts(*orbit.wide_table(), *W.offsets(view), exp2, mrd)
    assert np.array_equal(wc, pc), int((wc != pc).sum())
    assert np.array_equal(wm.view(np.uint64), pm.view(np.uint64))
    pick = np.random.RandomState(1).choice(wc.size, 150, replace=False)
    hc, hm = _host(orbit, view, pick, mrd)
    assert np.array_equal(hc, wc[pick]) and np.array_equal(hm.view(np.uint64), wm[pick].view(np.uint64))


# ---- the view, as Python names it -----------------------------------------------------------------------------------

def test_from_decimal_is_exact_and_rounds_once():
    from fractions import Fraction
    v = WideDeepView.from_decimal("1e-600", 64, 48)
    assert v.exp2 == -1994 and 1.0 <= v.range_r < 2.0 and (v.width, v.height) == (64, 48)
    exact = Fraction(1, 10 ** 600) * 2 ** 1994
    assert abs(Fraction(v.range_r) - exact) <= Fraction(np.spacing(v.range_r)) / 2
    assert v.range_i == v.range_r * 47 / 63 and v.min_span_exp2 == -1994
    assert WideDeepView.from_decimal("3", 8) == WideDeepView(3.0, 0, 8)
    assert WideDeepView.from_decimal("0.375", 8) == WideDeepView(1.5, -2, 8)
    assert WideDeepView.from_decimal(Decimal("1e-30"), 8).range_r == float(Fraction(1, 10 ** 30) * 2 ** 100)
    with pytest.raises(ValueError):
        WideDeepView.from_decimal("0", 8)
    assert DeepOrbit("0", "1", 10, min_span_exp2=-1100).precision_bits == 1216
    assert DeepOrbit("0", "1", 10, min_span_exp2=-5000).precision_bits == 4096
    with pytest.raises(ValueError):
        DeepOrbit("0", "1", 10, min_span=1e-3, min_span_exp2=-10)


# ---- refusals (the view's own; those that need a ctx are in tests/test_gpu_deep_wide.py) -----------------------------

def test_view_refusals_write_nothing():
    lib = L.load()
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    ok = dict(range_r=1.0, range_i=1.0, exp2=-50, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16)

    def call(mrd=50, col=3, row=4, **kw):
        f = dict(ok, **kw)
        cv = L.mbk_deep_xview(*[f[k] for k in ("range_r", "range_i", "exp2", "width", "height", "col0", "row0", "ncols", "nrows")])
        c, m = C.c_int32(-7), C.c_double(-7.0)
        st = lib.mbk_deep_xview_count_host(orbit._h, C.byref(cv), col, row, mrd, C.byref(c), C.byref(m))
        return st, c.value, m.value

    st, c, m = call()
    assert st == L.MBK_OK and (c, m) != (-7, -7.0)
    for lim in (dict(range_r=2.0 ** -64, range_i=4.0), dict(exp2=0), dict(exp2=-8192)):     # the limits themselves are accepted
        assert call(**lim)[0] == L.MBK_OK, lim
    bad = [dict(range_r=2.0 ** -65), dict(range_i=2.0 ** -65), dict(range_r=4.5), dict(range_i=float("inf")),
           dict(range_r=float("nan")), dict(range_r=0.0), dict(range_r=-1.0), dict(exp2=1), dict(exp2=-8193),
           dict(mrd=101), dict(ncols=0), dict(nrows=0), dict(col0=10, ncols=7), dict(row0=16, nrows=1),
           dict(width=0), dict(col=16), dict(row=16),
           dict(width=1 << 16, height=1 << 16, ncols=1 << 16, nrows=(1 << 15) + 1)]              # more than 2^31 pixels
    for kw in bad:
        assert call(**kw) == (L.MBK_ERR_INVALID, -7, -7.0), kw
    cv = L.mbk_deep_xview(1.0, 1.0, -50, 16, 16, 0, 0, 16, 16)
    c, m = C.c_int32(-7), C.c_double(-7.0)
    assert lib.mbk_deep_xview_count_host(None, C.byref(cv), 0, 0, 50, C.byref(c), C.byref(m)) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_count_host(orbit._h, None, 0, 0, 50, C.byref(c), C.byref(m)) == L.MBK_ERR_INVALID
    assert (c.value, m.value) == (-7, -7.0)


def test_struct_layout():
    assert C.sizeof(L.mbk_deep_xview) == 2 * 8 + 7 * 4 + 4      # padded to the alignment of its doubles
    assert L.mbk_deep_xview.exp2.offset == 16 and L.mbk_deep_xview.width.offset == 20


WIDE_RANGE = "extended-range deep view ranges must be finite and lie in [2^-64, 4]"
WIDE_EXP2 = "extended-range deep view exp2 must lie in [-8192, 0]"
# (what differs from a served call, the message); orbit mrd 100, view 16 x 16 of span 2^-50, pixel (3, 4), mrd 50
WIDE_REFUSALS = [
    (dict(orbit=None), "orbit is NULL"),
    (dict(view=None), "view is NULL"),
    (dict(width=0), "empty view"),
    (dict(height=0), "empty view"),
    (dict(ncols=0), "empty window"),
    (dict(nrows=0), "empty window"),
    (dict(col0=10, ncols=7), "window exceeds the view"),
    (dict(row0=16, nrows=1), "window exceeds the view"),
    (dict(width=1 << 16, height=1 << 16, ncols=1 << 16, nrows=(1 << 15) + 1), "window larger than 2^31 pixels"),
    (dict(range_r=2.0 ** -65), WIDE_RANGE),
    (dict(range_i=4.5), WIDE_RANGE),
    (dict(range_r=float("nan")), WIDE_RANGE),
    (dict(range_i=float("inf")), WIDE_RANGE),
    (dict(exp2=1), WIDE_EXP2),
    (dict(exp2=-8193), WIDE_EXP2),
    (dict(mrd=101), "mrd exceeds the mrd the reference orbit was computed for"),
    (dict(col=16), "pixel outside the view"),
    (dict(row=16), "pixel outside the view"),
    # two faults at once: the one reported
    (dict(orbit=None, range_r=float("nan")), "orbit is NULL"),
    (dict(width=0, mrd=101), "empty view"),
    (dict(range_r=8.0, exp2=1), WIDE_RANGE),
    (dict(exp2=1, mrd=101), WIDE_EXP2),
    (dict(mrd=101, col=16), "mrd exceeds the mrd the reference orbit was computed for"),
]


@pytest.mark.parametrize("change, message", WIDE_REFUSALS, ids=[",".join(c) for c, _ in WIDE_REFUSALS])
def test_validator_refusals_status_and_message(change, message):
    """Every line of the wide validator through the host-only call (no ctx: the calling thread's error text)."""
    from distributedmandelbrot_amd.device import _error_text
    lib = L.load()
    orbit = DeepOrbit("0", "1", 100, precision_bits=128)
    f = dict(dict(range_r=1.0, range_i=1.0, exp2=-50, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16), **change)
    cv = L.mbk_deep_xview(*[f[k] for k in ("range_r", "range_i", "exp2", "width", "height", "col0", "row0", "ncols", "nrows")])
    c, m = C.c_int32(-7), C.c_double(-7.0)
    st = lib.mbk_deep_xview_count_host(orbit._h if "orbit" not in change else None, C.byref(cv) if "view" not in change else None,
                                       f.get("col", 3), f.get("row", 4), f.get("mrd", 50), C.byref(c), C.byref(m))
    assert (st, _error_text(lib)) == (L.MBK_ERR_INVALID, message)
    assert (c.value, m.value) == (-7, -7.0)
