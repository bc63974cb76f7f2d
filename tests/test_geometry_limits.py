"""Views of up to 2^32 - 1 samples per axis on the host (no device): the reference for one axis sample (tests/geometry_model.py)
against np.linspace, the C oracle and exact rational arithmetic, and the host twins that take a view -- the literal-doubling
test, the outside-the-circle test, the MBK_OPT_SURE_INTERIOR counter and word, the units plan -- at view sizes and window
positions where a signed conversion, a 32-bit sum or a 32-bit product would show."""
import ctypes as C
import math

import numpy as np
import pytest

import geometry_model as G
from distributedmandelbrot_amd import _lib as L
from oracle.oracle import numpy_view

HUGE = [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 9, 2 ** 32 - 1]
AXES = [(-2.0, 4.0), (-0.7412314824132358 - 3.0, 3.0), (0.3, -1.7), (1e-3, 7e-10 * (2 ** 31)), (-1.5 * 2.0 ** -920, 3 * 2.0 ** -920)]


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- the reference itself -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 7, 4096, 65537, 10 ** 6])
@pytest.mark.parametrize("start,rng", AXES + [(0.25, 0.0), (0.0, 5e-324), (1.0, 1e-300), (-3.0, 2.0 ** -1070)])
def test_axis_sample_is_linspace(oracle, start, rng, n):
    """Every sample of axes of up to 10^6 samples, n = 1 and 2, a zero range and steps that round to zero among them (5e-324 / 2
    rounds to 0 while delta does not: numpy's step == 0 fallback; 1 + 1e-300 == 1: delta itself is 0)."""
    got = G.axis_sample(start, rng, n, np.arange(n, dtype=np.uint64))
    with np.errstate(all="ignore"):
        want = np.linspace(start, start + rng, n)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (start, rng, n)
    assert np.array_equal(got.view(np.uint64), oracle.axis(start, rng, n).view(np.uint64)), (start, rng, n)
    for k in {0, 1 % n, n // 2, n - 1}:
        assert G.axis_sample_exact(start, rng, n, k) == got[k], (start, rng, n, k)


def test_the_zero_step_cases_take_the_fallback():
    assert G._axis_facts(0.0, 5e-324, 3)[4] == 0.0 and G._axis_facts(0.0, 5e-324, 3)[2] != 0.0
    assert G._axis_facts(0.25, 0.0, 7)[4] == 0.0 and G._axis_facts(1.0, 1e-300, 7)[2] == 0.0


@pytest.mark.parametrize("n", HUGE)
@pytest.mark.parametrize("start,rng", AXES)
def test_axis_sample_against_exact_arithmetic(start, rng, n):
    """1000 seeded indices plus the ends and both sides of 2^31, against rational arithmetic rounded twice."""
    rs = np.random.RandomState(n % 1000003)
    ks = [int(k) for k in rs.randint(0, n, 1000, dtype=np.int64)] + [k for k in (0, 1, 2 ** 31 - 1, 2 ** 31, n - 2, n - 1) if k < n]
    got = G.axis_sample(start, rng, n, np.array(ks, dtype=np.uint64))
    for k, g in zip(ks, got):
        assert G.axis_sample_exact(start, rng, n, k) == g, (start, rng, n, k)
    assert got[-1] == np.float64(start) + np.float64(rng)


def test_view_window_is_the_window_of_the_whole_view():
    view = (-0.9, 0.05, 0.6, 0.45, 77, 53)
    for window in [None, (5, 7, 40, 30), (76, 52, 1, 1), (0, 10, 77, 3)]:
        cr, ci = G.view_window(view, window)
        col0, row0, ncols, nrows = window or (0, 0, 77, 53)
        assert np.array_equal(cr[0], np.linspace(-0.9, -0.9 + 0.6, 77)[col0:col0 + ncols])
        assert np.array_equal(ci[:, 0], np.linspace(0.05, 0.05 + 0.45, 53)[row0:row0 + nrows])
        counts, byts = G.window_counts(view, window, 60)
        wc, wb = numpy_view(*view, 60, window=window)
        assert np.array_equal(counts, wc) and np.array_equal(byts, wb)
        assert np.array_equal(G.window_escape(view, window, 60)[0], wc)


# ---- mbk_view_needs_literal_doubling ---------------------------------------------------------------------------------------------

SPAN = 2 ** 20


def _literal(lib, view, window, f32):
    cv = L.mbk_view(*view, *window)
    out = C.c_int(-1)
    assert lib.mbk_view_needs_literal_doubling(C.byref(cv), L.MBK_PRECISION_F32 if f32 else 0, C.byref(out)) == L.MBK_OK
    return int(out.value)


def _crossing(start, rng, n):
    """The row nearest the analytic zero of start + k * step, clipped to the axis."""
    step = G._axis_facts(start, rng, n)[4]
    return min(max(int(round(-start / step)), 0), n - 1) if step != 0.0 else 0


def _literal_model(start, rng, n, row0, nrows, f32):
    """Is a sample of rows [row0, row0 + nrows) tiny and non-zero?  From axis_sample on every row of the window within 2^20 rows of
    the zero crossing, plus the window's ends and the pinned last row.  The regular samples are monotone, so those nearest zero lie
    at the crossing: the span is asserted monotone, and to lie on both sides of zero when the window's ends do."""
    thr = 2.0 ** -100 if f32 else 2.0 ** -900
    k0 = _crossing(start, rng, n)
    lo, hi = max(row0, k0 - SPAN), min(row0 + nrows, k0 + SPAN + 1)
    ks = [row0, row0 + nrows - 1] + ([n - 1] if row0 + nrows == n else [])
    ks = np.concatenate([np.array(ks, dtype=np.uint64), np.arange(lo, max(hi, lo), dtype=np.uint64)])
    v = G.axis_sample(start, rng, n, ks)
    if f32:
        with np.errstate(all="ignore"):
            v = v.astype(np.float32).astype(np.float64)
    span = v[len(ks) - max(hi - lo, 0):]
    regular = span[:-1] if (hi == n and span.size) else span          # (the pinned last sample is no part of the sequence)
    d = np.diff(regular)
    assert (d >= 0).all() or (d <= 0).all(), (start, rng, n, row0, nrows)
    first, last = v[0], (G.axis_sample(start, rng, n, [row0 + nrows - 2])[0] if row0 + nrows == n and nrows > 1 else v[1])
    if first * last < 0:
        assert regular.size and regular.min() <= 0 <= regular.max(), "the crossing lies outside the span"
    return int(((v != 0.0) & (np.abs(v) < thr)).any())


LITERAL_AXES = [
    ("plain", -1.5, 3.0),                                   # samples near zero are ~1e-10: never tiny
    ("descending", 1.25, -3.0),
    ("tiny_at_the_crossing", -2.0 ** -880, 2.0 ** -879),    # step ~2^-910: tiny beside the crossing only, the ends are not
    ("all_tiny", -1.5 * 2.0 ** -920, 3 * 2.0 ** -920),
    ("f32_band", -1.5 * 2.0 ** -120, 3 * 2.0 ** -120),      # tiny for binary32 (below 2^-100) only; flushed to 0 below 2^-149
    ("ends_on_zero", -1.0, 1.0),                            # the pinned last sample is exactly 0
    ("ends_tiny", -2.0 ** -890, 2.0 ** -890 - 2.0 ** -940),  # the pinned last sample is -2^-940
]


@pytest.mark.parametrize("height", [2 ** 31 - 1, 2 ** 31 + 9, 2 ** 32 - 1])
def test_literal_doubling_at_huge_heights(lib, height):
    seen = {}
    for name, start, rng in LITERAL_AXES:
        k0 = _crossing(start, rng, height)
        windows = {"holds_the_crossing": (max(k0 - 3000, 0), min(6000, height - max(k0 - 3000, 0))),
                   "wide_over_the_crossing": (max(k0 - 2 ** 29, 0), min(2 ** 30, height - max(k0 - 2 ** 29, 0))),
                   "pinned_row_only": (height - 1, 1), "far_corner": (height - 11, 11), "first_rows": (0, 8),
                   "around_2^31": (2 ** 31 - 5, 21)}
        # the row before the first sample >= 0 (ascending) / <= 0 (descending), found from the model's own samples
        near = np.arange(max(k0 - 4, 0), min(k0 + 5, height - 1), dtype=np.uint64)
        vals = G.axis_sample(start, rng, height, near)
        neg = near[(vals < 0) if rng > 0 else (vals > 0)]
        if neg.size and 0 < k0 < height - 1:
            last_before = int(neg.max())
            windows["ends_one_row_before"] = (max(last_before - 999, 0), last_before - max(last_before - 999, 0) + 1)
        for wname, (row0, nrows) in windows.items():
            if row0 + nrows > height:
                continue
            for f32 in (False, True):
                want = _literal_model(start, rng, height, row0, nrows, f32)
                view = (-2.0, start, 4.0, rng, 1 << 12, height)
                # (the window is 1 column wide: up to 2^30 rows stay within the 2^31 pixels of a window)
                got = _literal(lib, view, (7, row0, 1, nrows), f32)
                assert got == want, (name, wname, height, row0, nrows, f32)
                seen.setdefault((wname, f32), set()).add(want)
    for wname in ("holds_the_crossing", "ends_one_row_before", "pinned_row_only", "wide_over_the_crossing"):
        assert seen[(wname, False)] == {0, 1} and seen[(wname, True)] == {0, 1}, (wname, seen)


# ---- the outside-the-circle test, the certificate's counter and word --------------------------------------------------------------

STEP = 7e-10


def _windows(w, h):
    # (an axis too short to hold index 2^31 + 15 takes its last 21 samples instead: up to index 2^31 - 2 or 2^31 - 1)
    return {"far_corner": (w - 24, h - 16, 24, 16), "ragged_far_corner": (w - 13, h - 11, 13, 11),
            "around_2^31": (min(2 ** 31 - 5, w - 21), min(2 ** 31 - 5, h - 21), 21, 21), "first_block": (0, 0, 8, 8),
            "before_the_edge": (w - 73, h - 41, 72, 40)}


def _outside_model(view, window, f32):
    xr, xi = G.window_axes(view, window)
    xlo, xhi, ylo, yhi = xr.min(), xr.max(), xi.min(), xi.max()
    dx = 0.0 if xlo <= 0.0 <= xhi else min(abs(xlo), abs(xhi))
    dy = 0.0 if ylo <= 0.0 <= yhi else min(abs(ylo), abs(yhi))
    return int(dx * dx + dy * dy >= 4.0 * (1.0 + (1e-4 if f32 else 1e-8)))


@pytest.mark.parametrize("w,h", [(2 ** 31 - 1, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 31 + 9), (2 ** 31, 2 ** 31)])
def test_outside_circle_at_the_corners_of_huge_views(lib, w, h):
    seen = set()
    for anchor in [(1.5, 1.5), (1.2, 1.2), (1.4142136, 1.4142136), (1.41421356, 1.41421356), (-1.4142137, 1.4142137), (1.9999999, 1e-9)]:
        for wname, window in _windows(w, h).items():
            if window[0] + window[2] > w or window[1] + window[3] > h:
                continue
            view = G.place_view(anchor, STEP, w, h, window)
            for f32 in (False, True):
                out = C.c_int(-1)
                cv = L.mbk_view(*view, *window)
                assert lib.mbk_view_outside_circle(C.byref(cv), L.MBK_PRECISION_F32 if f32 else 0, C.byref(out)) == L.MBK_OK
                want = _outside_model(view, window, f32)
                assert out.value == want, (anchor, wname, w, h, f32)
                seen.add((wname, want))
    assert {(n, v) for n in ("far_corner", "around_2^31", "first_block") for v in (0, 1)} <= seen


def _sure_point(cr, ci):
    """csrc/mbk_kernels.h sure_interior_point, every operation rounded on its own (numpy)."""
    ci2 = ci * ci
    x = cr - 0.25
    q = x * x + ci2
    xd = cr + 1.0
    return (q * (q + x) < 0.25 * ci2 - 1e-4) | (xd * xd + ci2 < 0.0625 - 1e-4)


def _blocks_model(view, window):
    """Whole 8x8 blocks of the window, free of a pinned last sample that the regular formula does not reproduce, all of whose 64
    pixels pass the certificate."""
    sr, si, rr, ri, w, h = view
    col0, row0, ncols, nrows = window
    ok = {}
    for name, (start, rng, n, k0, cnt) in {"re": (sr, rr, w, col0, ncols), "im": (si, ri, h, row0, nrows)}.items():
        regular_end = G.axis_sample(start, rng, n, [n - 1], pinned=False)[0] == G.axis_sample(start, rng, n, [n - 1])[0]
        n_ok = n if regular_end else n - 1
        ok[name] = min(cnt, n_ok - min(k0, n_ok)) // 8
    xr = G.axis_sample(sr, rr, w, np.uint64(col0) + np.arange(ok["re"] * 8, dtype=np.uint64), pinned=False)
    xi = G.axis_sample(si, ri, h, np.uint64(row0) + np.arange(ok["im"] * 8, dtype=np.uint64), pinned=False)
    acc = _sure_point(xr[None, :], xi[:, None])
    return int(acc.reshape(ok["im"], 8, ok["re"], 8).all(axis=(1, 3)).sum())


def _flag_model(view, window, mrd):
    xr, xi = G.window_axes(view, window)
    if mrd < 65 or not (xr.min() <= 0.4 and xr.max() >= -1.3 and xi.min() <= 0.7 and xi.max() >= -0.7):
        return 0
    ncols, nrows = window[2], window[3]
    pc = xr[[((2 * i + 1) * ncols) // 32 for i in range(16)]]
    pr = xi[[((2 * j + 1) * nrows) // 32 for j in range(16)]]
    return int(_sure_point(pc[None, :], pr[:, None]).any())


@pytest.mark.parametrize("w,h", [(2 ** 31 - 1, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 31 + 9), (2 ** 31, 2 ** 31)])
def test_sure_interior_counter_and_word_in_huge_views(lib, w, h):
    disk_edge = -1.0 + math.sqrt(0.0625 - 1e-4)        # the certificate's disk meets the real axis here
    seen_blocks, seen_flag = set(), set()
    for aname, anchor in {"inside": (-0.1, 0.1), "exterior": (0.5, 0.5), "disk_edge": (disk_edge - 12 * STEP, -8 * STEP),
                          "seahorse": (-0.7412314824132358, 0.11228268942084964)}.items():
        for wname, window in _windows(w, h).items():
            if window[0] + window[2] > w or window[1] + window[3] > h:
                continue
            view = G.place_view(anchor, STEP, w, h, window)
            cv = L.mbk_view(*view, *window)
            n, word = C.c_uint64(99), C.c_uint32(99)
            assert lib.mbk_sure_interior_blocks(C.byref(cv), C.byref(n)) == L.MBK_OK
            want = _blocks_model(view, window)
            assert n.value == want, (aname, wname, w, h, n.value, want)
            whole = (window[2] // 8) * (window[3] // 8)
            seen_blocks.add((aname, "none" if want == 0 else "all" if want == whole else "some"))
            for mrd in (64, 65, 1000):
                assert lib.mbk_sure_interior_flag(C.byref(cv), mrd, 0, 0, 1, C.byref(word)) == L.MBK_OK
                assert word.value == _flag_model(view, window, mrd), (aname, wname, w, h, mrd)
                seen_flag.add((aname, word.value))
    assert ("inside", "all") in seen_blocks and ("exterior", "none") in seen_blocks and ("disk_edge", "some") in seen_blocks
    assert ("inside", 1) in seen_flag and ("exterior", 0) in seen_flag and ("seahorse", 0) in seen_flag


# ---- the units plan at the largest list it accepts ---------------------------------------------------------------------------------

def _plan_model(n_h, n_v, n_m, fractions):
    """csrc/mbk_units.h units_plan and mbk_api.hip shares_from_fractions in unbounded integers."""
    cum, c = [], 0.0
    for x in range(8):
        c += fractions[x]
        cum.append(1 << 24 if x == 7 else int(round(min(1.0, max(0.0, c)) * (1 << 24))))
    n_l, total = n_m + n_v, n_h + n_m + n_v
    h, prev, slots = [], 0, (total + 7) >> 3
    for x in range(8):
        cc = n_h if x == 7 else (n_h * cum[x]) >> 24
        cc = max(prev, min(cc, n_h))
        h.append(cc - prev)
        prev = cc
        slots = max(slots, h[x])
    left, lgt = n_l, []
    for x in range(8):
        lgt.append(min(slots - h[x], left))
        left -= lgt[x]
    hmin, lmin = min(h), min(lgt)
    hb, lb, hbase, lbase = 8 * hmin, 8 * lmin, [], []
    for x in range(8):
        hbase.append(hb - hmin)
        lbase.append(lb - lmin)
        hb += h[x] - hmin
        lb += lgt[x] - lmin
    return dict(total=slots * 8, h=h, l=lgt, hmin=hmin, lmin=lmin, hbase=hbase, lbase=lbase, n_m=n_m)


def _lookup_model(p, u):
    """(list, index): 1 = heavy, 2 = middle, 3 = row units, 0 = none."""
    x, j = u & 7, u >> 3
    if j < p["h"][x]:
        return 1, (u if j < p["hmin"] else p["hbase"][x] + j)
    k = j - p["h"][x]
    if k >= p["l"][x]:
        return 0, 0
    i = 8 * k + x if k < p["lmin"] else p["lbase"][x] + k
    return (2, i) if i < p["n_m"] else (3, i - p["n_m"])


@pytest.mark.parametrize("n_h,n_v,n_m", [(2 ** 30, 2 ** 30 - 6, 5), (2 ** 31 - 1, 0, 0), (0, 2 ** 31 - 1, 0), (7, 2 ** 30, 2 ** 30 - 8),
                                         (2 ** 31 - 3, 1, 1)])
@pytest.mark.parametrize("fractions", [[0.125] * 8, [0.110, 0.140, 0.125, 0.120, 0.130, 0.125, 0.115, 0.135], [0.14, 0.11] * 4])
def test_units_plan_at_the_largest_list(lib, n_h, n_v, n_m, fractions):
    """n_h + n_v + n_m = 2^31 - 1, the most mbk_units_plan accepts: 10^5 ids, both ends of the id range among them, each map to
    the entry the same arithmetic gives in unbounded integers -- so to one entry inside its list, distinct ids to distinct ones."""
    assert n_h + n_v + n_m == 2 ** 31 - 1
    plan = (C.c_uint32 * 40)()
    assert lib.mbk_units_plan(n_h, n_v, n_m, (C.c_double * 8)(*fractions), plan) == 0
    model = _plan_model(n_h, n_v, n_m, fractions)
    assert plan[2] == model["total"] and plan[2] % 8 == 0 and plan[2] >= 2 ** 31 - 1
    assert list(plan[8:16]) == model["h"] and list(plan[16:24]) == model["l"]
    assert sum(plan[8:16]) == n_h and sum(plan[16:24]) == n_v + n_m
    total = int(plan[2])
    rs = np.random.RandomState(11)
    ids = set(range(0, 64)) | set(range(total - 64, total)) | {u for u in (2 ** 30 - 1, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1) if u < total}
    ids |= {int(u) for u in rs.randint(0, total, 100000 - len(ids), dtype=np.int64)}
    li, ix = C.c_uint32(), C.c_uint32()
    entries = set()
    sizes = {1: n_h, 2: n_m, 3: n_v}
    for u in sorted(ids):
        assert lib.mbk_units_lookup(plan, u, C.byref(li), C.byref(ix)) == 0
        assert (li.value, ix.value) == _lookup_model(model, u), u
        if li.value:
            assert ix.value < sizes[li.value], (u, li.value, ix.value)
            assert (li.value, ix.value) not in entries, u
            entries.add((li.value, ix.value))
    assert len(entries) > 50000        # (ids beyond an XCD's shares compute nothing: the uneven deals leave some)


def test_units_plan_refuses_2_to_the_31(lib):
    plan = (C.c_uint32 * 40)()
    f = (C.c_double * 8)(*([0.125] * 8))
    for n_h, n_v, n_m in [(2 ** 30, 2 ** 30, 0), (2 ** 31, 0, 0), (0, 1, 2 ** 31 - 1), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)]:
        assert lib.mbk_units_plan(n_h, n_v, n_m, f, plan) == L.MBK_ERR_INVALID, (n_h, n_v, n_m)
