"""Interior views on the host (include/mbk.h, "Interior views"): mbk_interior_host and mbk_interior_resolve_host -- compiled from
the functions the kernel and the resolve kernel use -- held to the numpy model of the contract (tests/interior_model.py), and the
contract itself held to the two components whose boundaries are known in closed form (tests/test_interior_truth.py holds the
value of de to the mathematics).  The hazard views -- rows with a subnormal c_i, where the fused doubling of the kernels would
find other cycles -- are tabled here for the GPU tests, with the claims those rest on.

Measured with the model on the 160 x 160 grid of [-2, 1] x [-1.5, 1.5] at mrd 4096: 4002 settled pixels, 3168 of them in the
cardioid and 518 in the period-2 disc; period 1 on every cardioid pixel and 2 on every disc pixel, the period divides the cycle
length everywhere, and de / true distance lies in [1.174, 3.290] on the cardioid and [1.038, 1.967] on the disc (Koebe: [1, 4])."""
import ctypes as C
import math

import numpy as np
import pytest

import interior_model as M
import interior_truth as T
from distributedmandelbrot_amd import MbkError
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import interior_host, interior_resolve_host

FULL = (-2.0, -1.5, 3.0, 3.0)

# Hazard views: rows with 0 < |c_i| < 2^-900, where zi stays subnormal and the fused doubling fma(2, zr zi, c_i) rounds
# differently from the contract's literal fl(fl(2 zr) zi) + c_i.  The counts are the same, but the cycle stage is a bit compare:
# the two forms reach the bitwise repeat at different steps, and period and de follow.  A launch must take the literal kernel on
# these views; the host twin always does.  (view, {mrd: pixels on which the fused model differs in period or de}) -- the mrd
# lie just past a Brent window edge; from mrd 300 on the differences are gone on all but the first view, and the third has none
# left at mrd 257, which is why that pair is not here.  test_hazard_claims asserts every figure.
HAZARD_MIXED = (-2.0, 1e-310, 2.5, 0.7, 96, 8)      # row 0 alone is tiny: rows 1..7 are 0.1 .. 0.7
HAZARD = [
    ((-2.0, 1e-310, 2.5, 3e-310, 96, 8), {33: 12, 65: 23, 129: 14, 257: 13}),      # every row tiny
    (HAZARD_MIXED, {33: 2, 65: 4, 129: 2, 257: 3}),                                # all in row 0
    ((-1.5, -3e-323, 1.9, 6e-323, 29, 13), {33: 2, 65: 24, 129: 10}),              # rows of -6 .. 6 units of 2^-1074, row 6 is 0
    ((-2.0, 1e-310, 2.5, 0.0, 96, 1), {33: 2, 65: 4, 129: 2, 257: 3}),             # one row, zero range
    ((-2.0, -3e-310, 2.5, 6e-310, 96, 7), {33: 10, 65: 20, 129: 10, 257: 16}),     # rows on both sides of zero, row 3 is 0
]
HAZARD_CASES = [(v, mrd) for v, table in HAZARD for mrd in table]


def differing_pixels(a, b):
    """How many pixels of two results (dicts of arrays, or (period, de) pairs) differ in period or in the bits of de."""
    (pa, da), (pb, db) = ((x["period"], x["de"]) if isinstance(x, dict) else x for x in (a, b))
    return int(((pa != pb) | (np.ascontiguousarray(da).view(np.uint64) != np.ascontiguousarray(db).view(np.uint64))).sum())


def _host(cr, ci, mrd):
    got = [interior_host((float(a), float(b)), mrd) for a, b in zip(np.ravel(cr), np.ravel(ci))]
    return (np.array([g[0] for g in got], np.int32), np.array([g[1] for g in got], np.int32),
            np.array([g[2] for g in got], np.int32), np.array([g[3] for g in got], np.float64))


def _assert_equals_model(cr, ci, mrd, what):
    n, p, cl, de = _host(cr, ci, mrd)
    m = M.interior(cr, ci, mrd)
    assert np.array_equal(n, m["n"]), what
    assert np.array_equal(p, m["period"]), what
    assert np.array_equal(cl, m["cycle"]), what
    assert np.array_equal(de.view(np.uint64), m["de"].view(np.uint64)), what
    assert not np.isnan(de).any() and (de >= 0.0).all(), what
    return m


def test_host_equals_the_model_on_a_grid():
    v = FULL + (64, 64)
    xr, xi = M.axes(v)
    cr, ci = np.meshgrid(xr, xi)
    m = _assert_equals_model(cr, ci, 1500, "grid")
    inside = m["n"] == 0
    assert 500 < int(inside.sum()) < 1000 and (m["period"][~inside] == 0).all() and (m["de"][~inside] == 0.0).all()
    assert (m["period"][inside] > 0).sum() > 500 and (m["period"][inside] == 0).any()      # settled and unknown pixels
    assert len(np.unique(m["period"])) >= 4 and (m["cycle"] > m["period"]).any()            # the bitwise period is a proper multiple


def test_hand_cases():
    assert interior_host((0.0, 0.0), 100) == (0, 1, 1, 0.5)
    assert interior_host((0.0, 0.0), 2) == (0, 1, 1, 0.5)
    for mrd in (4, 5, 100):
        assert interior_host((-1.0, 0.0), mrd) == (0, 2, 2, 0.25)
    assert interior_host((-1.0, 0.0), 3) == (0, 0, 0, 0.0)                                  # unknown
    for c in ((0.0, 0.0), (-1.0, 0.0)):
        m = M.interior([c[0]], [c[1]], 100)
        assert (int(m["n"][0]), int(m["period"][0]), int(m["cycle"][0]), float(m["de"][0])) == interior_host(c, 100)
        assert m["at_window"][0]                          # the hit falls on a step with since == w: the hit is taken first
    assert interior_host((2.0, 2.0), 100)[:3] == (1, 0, 0)


def test_signed_zero_is_a_bit_compare():
    """c = (-1, -0): z_2 = (-1, +0) equals z_0 in value and not in bits, so the cycle 0 <-> -1 is found two steps later."""
    m = _assert_equals_model([-1.0], [-0.0], 100, "-0")
    plus = M.interior([-1.0], [0.0], 100)
    assert int(m["period"][0]) == 2 and float(m["de"][0]) == 0.25 and int(m["cycle"][0]) != int(plus["cycle"][0])


@pytest.mark.parametrize("mrd", [0, 1, 2])
def test_shallow_mrd(mrd):
    xr, xi = M.axes(FULL + (9, 9))
    cr, ci = np.meshgrid(xr, xi)
    m = _assert_equals_model(cr, ci, mrd, f"mrd {mrd}")
    if mrd < 2:
        assert not m["n"].any() and not m["period"].any() and not m["de"].any()


@pytest.mark.parametrize("v,table", HAZARD, ids=[str(i) for i in range(len(HAZARD))])
def test_host_equals_the_literal_model_on_the_hazard_views(v, table):
    xr, xi = M.axes(v)
    cr, ci = np.meshgrid(xr, xi)
    assert ((xi != 0.0) & (np.abs(xi) < 2.0 ** -900)).any()
    for mrd in table:
        m = _assert_equals_model(cr, ci, mrd, (v, mrd))
        assert (m["period"] > 0).any() and (m["n"] > 0).any()


@pytest.mark.parametrize("v,table", HAZARD, ids=[str(i) for i in range(len(HAZARD))])
def test_hazard_claims(v, table):
    """What the GPU tests of the hazard views rest on: with the fused doubling the counts are the same and period or de are not,
    on exactly the number of pixels the table records -- so a launch that took the fused kernel would show."""
    assert table
    for mrd, want in table.items():
        lit, fused = M.view(v, mrd), M.view(v, mrd, fma=True)
        assert np.array_equal(lit["n"], fused["n"]), (v, mrd)
        diff = differing_pixels(lit, fused)
        print(f"{v} mrd {mrd}: the fused model differs on {diff} pixels")
        assert diff == want and diff >= 1, (v, mrd, diff)
    if v == HAZARD_MIXED:      # rows 1..7 are ordinary: the two forms agree there, and all the differences lie in row 0
        for mrd in table:
            lit, fused = M.view(v, mrd, window=(0, 1, 96, 7)), M.view(v, mrd, window=(0, 1, 96, 7), fma=True)
            assert differing_pixels(lit, fused) == 0 and np.array_equal(lit["cycle"], fused["cycle"])


def test_fused_model_is_the_literal_one_on_ordinary_views():
    """The fma option changes nothing where no row is tiny, cycle lengths included."""
    v = FULL + (64, 64)
    lit, fused = M.view(v, 300), M.view(v, 300, fma=True)
    for k in lit:
        assert np.array_equal(lit[k].view(np.uint64) if k == "de" else lit[k], fused[k].view(np.uint64) if k == "de" else fused[k]), k


def test_guard_says_literal_for_every_hazard_view():
    lib = L.load()

    def guard(v, window=None):
        c0, r0, nc, nr = window or (0, 0, v[4], v[5])
        cv = L.mbk_view(v[0], v[1], v[2], v[3], v[4], v[5], c0, r0, nc, nr)
        out = C.c_int(-1)
        assert lib.mbk_view_needs_literal_doubling(C.byref(cv), 0, C.byref(out)) == L.MBK_OK
        return out.value

    for v, _ in HAZARD:
        assert guard(v) == 1, v
    assert guard(HAZARD_MIXED, (0, 0, 96, 1)) == 1 and guard(HAZARD_MIXED, (5, 0, 40, 3)) == 1
    assert guard(HAZARD_MIXED, (0, 1, 96, 7)) == 0
    assert guard(FULL + (64, 64)) == 0 and guard(FULL + (61, 45)) == 0


@pytest.fixture(scope="module")
def grid160():
    return T.model_case(T.GRID160)      # (shared with tests/test_interior_truth.py: computed once)


def _polyline_distance(px, py, bx, by):
    """The distance of every point to the closed polyline through (bx, by)."""
    ax, ay, dx, dy = bx[:-1], by[:-1], np.diff(bx), np.diff(by)
    len2 = dx * dx + dy * dy
    best = np.full(px.size, np.inf)
    for lo in range(0, px.size, 256):
        x, y = px[lo:lo + 256, None], py[lo:lo + 256, None]
        t = np.clip(((x - ax) * dx + (y - ay) * dy) / len2, 0.0, 1.0)
        best[lo:lo + 256] = np.sqrt(((x - (ax + t * dx)) ** 2 + (y - (ay + t * dy)) ** 2).min(axis=1))
    return best


def test_components(grid160):
    """The cardioid and the period-2 disc: periods 1 and 2, the period divides the cycle length, Koebe's bounds."""
    cr, ci, m = grid160
    settled = m["period"] > 0
    q = (cr - 0.25) ** 2 + ci * ci
    cardioid = settled & (q * (q + (cr - 0.25)) < 0.25 * ci * ci)
    disc = settled & ((cr + 1.0) ** 2 + ci * ci < 1.0 / 16.0)
    print(f"settled {int(settled.sum())}, cardioid {int(cardioid.sum())}, disc {int(disc.sum())}")
    assert int(settled.sum()) >= 3900 and int((cardioid | disc).sum()) >= 3500
    assert (m["period"][cardioid] == 1).all()
    assert (m["period"][disc] == 2).all()
    assert (m["cycle"][settled] % m["period"][settled] == 0).all()
    assert (m["cycle"][cardioid] > 1).any()               # which is why the cycle test cannot give the period
    th = np.linspace(0.0, 2.0 * np.pi, 20001)
    for name, sel, bx, by in (("cardioid", cardioid, 0.5 * np.cos(th) - 0.25 * np.cos(2 * th), 0.5 * np.sin(th) - 0.25 * np.sin(2 * th)),
                              ("disc", disc, -1.0 + 0.25 * np.cos(th), 0.25 * np.sin(th))):
        ratio = m["de"][sel] / _polyline_distance(cr[sel], ci[sel], bx, by)
        print(f"{name}: de / true distance in [{ratio.min():.3f}, {ratio.max():.3f}]")
        assert ratio.min() >= 0.99 and ratio.max() <= 4.01, name


def test_host_equals_the_model_on_component_pixels(grid160):
    """A seeded sample of the deep grid through the host twin: long cycles, periods above 2, unknown pixels."""
    cr, ci, m = grid160
    inside = np.flatnonzero(m["n"] == 0)
    pick = np.concatenate([np.random.RandomState(3).choice(inside, 150, replace=False), np.flatnonzero(m["period"] > 2)[:50],
                           np.flatnonzero((m["n"] == 0) & (m["period"] == 0))[:10]])
    n, p, cl, de = _host(cr[pick], ci[pick], 4096)
    assert np.array_equal(n, m["n"][pick]) and np.array_equal(p, m["period"][pick]) and np.array_equal(cl, m["cycle"][pick])
    assert np.array_equal(de.view(np.uint64), m["de"][pick].view(np.uint64))


def _samples(h, w, seed):
    rs = np.random.RandomState(seed)
    n = np.where(rs.rand(h, w) < 0.3, rs.randint(1, 50, (h, w)), 0).astype(np.int32)
    period = np.where((n == 0) & (rs.rand(h, w) < 0.9), rs.randint(1, 40, (h, w)), 0).astype(np.int32)
    de = np.where(period > 0, rs.rand(h, w) * 0.01, 0.0)
    de.ravel()[::17] = np.where(period.ravel()[::17] > 0, math.inf, 0.0)
    de.ravel()[5::13] = 0.0
    return n, period, de


@pytest.mark.parametrize("plen", [1, 7])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_resolve_host_equals_the_model(s, plen):
    h, w = 11, 13
    n, period, de = _samples(h * s, w * s, 10 * s + plen)
    pal = np.random.RandomState(plen).randint(0, 256, (plen, 4)).astype(np.uint8)
    unknown, outside = (1, 2, 3, 4), (250, 251, 252, 253)
    assert (period > plen).any() and np.isinf(de).any() and ((period > 0) & (de == 0.0)).any() and ((n == 0) & (period == 0)).any()
    for scale in (2.0 ** 80, 150.0, 1.0 / 0.01):      # the flat map and two ramps
        got = interior_resolve_host(n, period, de, palette=pal, supersample=s, scale=scale, unknown=unknown, outside=outside)
        want = M.render(pal, unknown, outside, scale, s, n, period, de)
        assert got.shape == (h, w, 4) and np.array_equal(got, want), (s, plen, scale)
    if s == 1:
        flat = interior_resolve_host(n, period, de, palette=pal, scale=2.0 ** 80, unknown=unknown, outside=outside)
        lit = (period > 0) & (de > 0.0)
        assert np.array_equal(flat[lit], pal[(period[lit] - 1) % plen])               # the period map
        dark = (period > 0) & (de == 0.0)
        assert (flat[dark][:, :3] == 0).all() and np.array_equal(flat[dark][:, 3], pal[(period[dark] - 1) % plen][:, 3])
        assert (flat[n > 0] == outside).all() and (flat[(n == 0) & (period == 0)] == unknown).all()


def test_refusals_of_the_host_calls():
    lib = L.load()
    n, p, cl, de = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_double(7.0)
    assert lib.mbk_interior_host(0.0, 0.0, 100, None, C.byref(p), C.byref(cl), C.byref(de)) == L.MBK_ERR_INVALID
    assert lib.mbk_interior_host(0.0, 0.0, 2 ** 31, C.byref(n), C.byref(p), C.byref(cl), C.byref(de)) == L.MBK_ERR_INVALID
    assert (n.value, p.value, cl.value, de.value) == (7, 7, 7, 7.0)
    assert lib.mbk_interior_host(0.0, 0.0, 100, C.byref(n), None, None, None) == L.MBK_OK and n.value == 0
    with pytest.raises(MbkError):
        interior_host((0.0, 0.0), 2 ** 31)
    cnt, per, d = _samples(8, 8, 1)
    pal = np.full((3, 4), 9, np.uint8)
    for bad in (dict(supersample=5), dict(supersample=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=2.0 ** 81), dict(scale=math.inf),
                dict(scale=math.nan), dict(palette=np.zeros((0, 4), np.uint8)), dict(palette=np.zeros((65537, 4), np.uint8))):
        with pytest.raises(MbkError):
            interior_resolve_host(cnt, per, d, **{"palette": pal, **bad})
    spec = L.mbk_interior_render_spec(1, pal.ctypes.data, 3, (C.c_uint8 * 4)(), (C.c_uint8 * 4)(), 1.0, 0)
    out = np.full((8, 8, 4), 7, np.uint8)
    args = (cnt.ctypes.data, per.ctypes.data, d.ctypes.data)
    resolve = lib.mbk_interior_resolve_host
    assert resolve(None, 8, 8, *args, out.ctypes.data) == L.MBK_ERR_INVALID
    assert resolve(C.byref(spec), 8, 8, *args, None) == L.MBK_ERR_INVALID
    assert resolve(C.byref(spec), 0, 8, *args, out.ctypes.data) == L.MBK_ERR_INVALID
    assert resolve(C.byref(spec), 8, 2 ** 31, *args, out.ctypes.data) == L.MBK_ERR_INVALID
    for k in range(3):
        a = list(args)
        a[k] = None
        assert resolve(C.byref(spec), 8, 8, *a, out.ctypes.data) == L.MBK_ERR_INVALID
    assert (out == 7).all()
    assert resolve(C.byref(spec), 8, 8, *args, out.ctypes.data) == L.MBK_OK
