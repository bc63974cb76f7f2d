"""Deep-zoom views with bilinear approximation on the CPU (include/mbk.h, "Deep-zoom views with bilinear approximation"):
the library's table and its one-pixel host twin (compiled from the functions the builder and the kernel use) against the
numpy restatement (tests/deep_bla_model.py), and that restatement against the truth -- z = z^2 + c iterated directly in
fixed point at P + 128 fraction bits -- under the cap tests/test_deep_truth.py already uses."""
import ctypes as C
import functools

import numpy as np
import pytest

import deep_bla_model as B
import deep_model as D
from test_deep_truth import CASES, M51

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
# the catalogue of tests/test_deep_truth.py as (centre, span_r, span_i, mrd, pixels), and the seahorse view of tests/test_gpu_deep.py
TRUTH_CASES = [(c, sr, si, mrd, 150) for c, sr, si, mrd, _, _ in CASES] + [(SEAHORSE, 1e-20, None, 30000, 80)]
IDS = [f"{c[0][:10]}-{sr:g}" for c, sr, _, _, _ in TRUTH_CASES]


def _lib():
    from distributedmandelbrot_amd import _lib as L
    return L, L.load()


def _cview(L, view):
    return L.mbk_deep_view(view.span_r, view.span_i, view.width, view.height, 0, 0, view.width, view.height)


def _read_table(orbit, view):
    """The library's table: a list of levels, each (Ar, Ai, Br, Bi, rc)."""
    L, lib = _lib()
    cv = _cview(L, view)
    levels, entries = C.c_uint32(), C.c_uint64()
    assert lib.mbk_deep_bla_info(orbit._h, C.byref(cv), C.byref(levels), C.byref(entries)) == L.MBK_OK
    out = []
    for l in range(levels.value):
        n = (orbit.length - 1) >> l
        arrays = [np.full(n, -7.0) for _ in range(5)]
        assert lib.mbk_deep_bla_read(orbit._h, C.byref(cv), l, *[a.ctypes.data for a in arrays], n) == L.MBK_OK
        out.append(arrays)
    assert sum(a[0].size for a in out) == entries.value
    return out


def _host_counts(orbit, view, pick, mrd):
    L, lib = _lib()
    cv = _cview(L, view)
    c, mg, st = np.empty(pick.size, np.int32), np.empty(pick.size), np.empty(pick.size, np.int64)
    for n, p in enumerate(pick):
        cc, mm, ss = C.c_int32(), C.c_double(), C.c_uint64()
        assert lib.mbk_deep_bla_count_host(orbit._h, C.byref(cv), int(p % view.width), int(p // view.width), mrd,
                                           C.byref(cc), C.byref(mm), C.byref(ss)) == L.MBK_OK
        c[n], mg[n], st[n] = cc.value, mm.value, ss.value
    return c, mg, st


@functools.lru_cache(maxsize=None)
def _case(k):
    """One case of TRUTH_CASES, computed once: the orbit, the view, the sampled pixels, the BLA model and the plain model."""
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    centre, span_r, span_i, mrd, pixels = TRUTH_CASES[k]
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i or span_r))
    view = DeepView(span_r, 64, 64, span_i)
    dr, di = D.offsets(view)
    pick = np.random.RandomState(1).choice(dr.size, pixels, replace=False)
    zr, zi = orbit.table()
    table = B.build(zr, zi, B.dcmax(view))
    c, mg, st = B.counts(zr, zi, dr[pick], di[pick], mrd, table)
    pc, pm = D.model_counts(zr, zi, dr[pick], di[pick], mrd)
    return dict(centre=centre, mrd=mrd, orbit=orbit, view=view, pick=pick, dr=dr[pick], di=di[pick], zr=zr, zi=zi,
                count=c, mag=mg, steps=st, plain=pc, plain_mag=pm)


@functools.lru_cache(maxsize=None)
def _truth(k):
    s = _case(k)
    return D.direct_counts(s["centre"][0], s["centre"][1], s["dr"], s["di"], s["mrd"], s["orbit"].precision_bits + 128)


def _same_bits(a, b):
    """Bit for bit; where an overflowed product left a NaN, a NaN (its sign and payload are the host's business)."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


# 1. the table
@pytest.mark.parametrize("span", [1e-30, 2.0 ** -960, 4.0], ids=["1e-30", "2^-960", "4"])
@pytest.mark.parametrize("centre, mrd, M", [(("0", "1"), 3000, 3000), (("1e-21", "1"), 5000, 58), (("0", "0"), 100, 100)])
def test_table_equals_the_model(centre, mrd, M, span):
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    orbit = DeepOrbit(*centre, mrd, min_span=1e-30)
    assert orbit.length == M
    view = DeepView(span, 64, 48, span)
    zr, zi = orbit.table()
    model = B.build(zr, zi, B.dcmax(view))
    got = _read_table(orbit, view)
    assert len(got) == len(model) == (M - 1).bit_length()
    for l, (lv, arrays) in enumerate(zip(model, got)):
        assert lv["rc"].size == (M - 1) >> l
        for name, a in zip(("Ar", "Ai", "Br", "Bi", "rc"), arrays):
            assert _same_bits(lv[name], a), (l, name)
        assert (lv["rc"] >= 0.0).all()
    rc = [lv["rc"] for lv in model]
    for l in range(1, len(rc)):                     # r does not grow with the level at a fixed starting m
        assert (rc[l] <= rc[l - 1][0:2 * rc[l].size:2]).all(), l
    if centre == ("0", "0"):
        assert all((r == 0.0).all() for r in rc)    # every Z is 0: nothing may ever be skipped
    elif span == 4.0:
        assert all((r == 0.0).all() for r in rc[1:])
    else:
        assert (rc[0] > 0.0).all() and (rc[1] > 0.0).any()
    if centre == ("0", "1") and span != 4.0:        # |A| grows like 4^(2^l): the highest levels overflowed and are never taken
        top = model[-1]
        assert not np.isfinite(top["Ar"]).all() or not np.isfinite(top["Ai"]).all()
        assert (top["rc"] == 0.0).all()


def test_table_calls_refuse_what_they_cannot_serve():
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    L, lib = _lib()
    one = DeepOrbit("-2", "0", 100, min_span=1e-10)
    cv = _cview(L, DeepView(1e-10, 8))
    levels, entries = C.c_uint32(9), C.c_uint64(9)
    assert lib.mbk_deep_bla_info(one._h, C.byref(cv), C.byref(levels), C.byref(entries)) == L.MBK_OK
    assert (one.length, levels.value, entries.value) == (1, 0, 0)             # M = 1: no table
    a = np.empty(4)
    p = [a.ctypes.data] * 5
    assert lib.mbk_deep_bla_read(one._h, C.byref(cv), 0, *p, 4) == L.MBK_ERR_INVALID
    orbit = DeepOrbit("0", "1", 100, min_span=1e-10)
    assert lib.mbk_deep_bla_read(orbit._h, C.byref(cv), 0, *p, 4) == L.MBK_ERR_INVALID      # 99 entries do not fit 4
    assert lib.mbk_deep_bla_read(orbit._h, C.byref(cv), 7, *p, 4) == L.MBK_ERR_INVALID      # levels 0 .. 6
    assert lib.mbk_deep_bla_read(None, C.byref(cv), 0, *p, 4) == L.MBK_ERR_INVALID
    cc, mm, ss = C.c_int32(), C.c_double(), C.c_uint64()
    assert lib.mbk_deep_bla_count_host(orbit._h, C.byref(cv), 8, 0, 100, C.byref(cc), C.byref(mm), C.byref(ss)) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_bla_count_host(orbit._h, C.byref(cv), 0, 0, 101, C.byref(cc), C.byref(mm), C.byref(ss)) == L.MBK_ERR_INVALID


# 2. the stepping
@pytest.mark.parametrize("k", range(len(TRUTH_CASES)), ids=IDS)
def test_host_twin_equals_the_model(k):
    s = _case(k)
    c, mg, st = _host_counts(s["orbit"], s["view"], s["pick"], s["mrd"])
    assert np.array_equal(c, s["count"]), int((c != s["count"]).sum())
    assert np.array_equal(mg.view(np.uint64), s["mag"].view(np.uint64))
    assert np.array_equal(st, s["steps"])


@pytest.mark.parametrize("mrd", [0, 1, 2, 3, 4, 5, 6, 9, 10, 17, 18, 33, 34, 257, 258])
def test_host_twin_at_the_end_of_the_loop(mrd):
    """i + 2^l <= mrd: launches whose mrd ends on a skip boundary, one above it and one below it."""
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    orbit = DeepOrbit("0", "1", 3000, min_span=1e-200)
    view = DeepView(1e-200, 9, 7)
    zr, zi = orbit.table()
    dr, di = D.offsets(view)
    c, mg, st = B.counts(zr, zi, dr, di, mrd, B.build(zr, zi, B.dcmax(view)))
    hc, hm, hs = _host_counts(orbit, view, np.arange(63), mrd)
    assert np.array_equal(hc, c) and np.array_equal(hm, mg) and np.array_equal(hs, st)
    assert not c.any()                                        # nothing escapes this early at c = i
    if mrd >= 2:                                              # steps 1 .. mrd-1 in as few skips as their binary form has
        assert (st == bin(mrd - 1).count("1")).all(), st


# 3. the truth
@pytest.mark.parametrize("k", range(len(TRUTH_CASES)), ids=IDS)
def test_model_equals_direct_iteration(k):
    s = _case(k)
    truth = _truth(k)
    assert len(np.unique(truth)) >= 8, np.unique(truth)
    assert (s["count"] == truth).mean() >= 0.99, (int((s["count"] != truth).sum()), np.unique(s["count"]), np.unique(truth))


def test_eps_2_to_the_minus_24_fails_the_cap_on_the_seahorse_view():
    """Why eps is 2^-40: the tolerance the literature suggests for binary64 misses this project's truth."""
    k = len(TRUTH_CASES) - 1
    s = _case(k)
    loose = B.build(s["zr"], s["zi"], B.dcmax(s["view"]), eps=2.0 ** -24)
    c, _, st = B.counts(s["zr"], s["zi"], s["dr"], s["di"], s["mrd"], loose)
    assert (c == _truth(k)).mean() < 0.99
    assert st.sum() < s["steps"].sum()                       # it does skip more


# 4. it skips
def _plain_total(s):
    return int(np.where(s["plain"] > 0, s["plain"], s["mrd"] - 1).astype(np.int64).sum())


@pytest.mark.parametrize("centre, span", [(("0", "1"), 1e-30), (M51, 1e-35)], ids=["i-1e-30", "M51-1e-35"])
def test_steps_executed_at_most_half(centre, span):
    k = [n for n, t in enumerate(TRUTH_CASES) if t[0] == centre and t[1] == span][0]
    s = _case(k)
    _, _, st = _host_counts(s["orbit"], s["view"], s["pick"], s["mrd"])
    assert 2 * int(st.sum()) <= _plain_total(s), (int(st.sum()), _plain_total(s))


def test_no_table_no_skip():
    k = [n for n, t in enumerate(TRUTH_CASES) if t[0] == ("-2", "0")][0]
    s = _case(k)
    assert s["orbit"].length == 1
    c, mg, st = _host_counts(s["orbit"], s["view"], s["pick"], s["mrd"])
    assert int(st.sum()) == _plain_total(s)
    assert np.array_equal(c, s["plain"]) and np.array_equal(mg, s["plain_mag"])


# 5. without the flag
def test_the_plain_contract_is_untouched():
    """The flag is a bit no other flag uses, and deep_model.model_counts -- what mbk_deep_* compute without it
    (tests/test_gpu_deep.py; tests/test_gpu_deep_bla.py runs one case beside the flag) -- is what it was: equal to the truth
    on a case of tests/test_deep_truth.py, from the same orbit table the BLA model reads."""
    from distributedmandelbrot_amd import _lib as L
    taken = L.MBK_WANT_COUNTS | L.MBK_WANT_BYTES | 0xF00 | L.MBK_PRECISION_F32 | L.MBK_LAZY_UNIFORM
    assert L.MBK_DEEP_BLA == 0x8000 and not L.MBK_DEEP_BLA & taken
    s = _case(1)
    assert np.array_equal(s["plain"], _truth(1))


# ---- the refusals of the deep validator, line by line, through the host-only calls (no ctx: the calling thread's text) ----

RANGE = "deep view ranges must be finite and lie in [2^-960, 4]"
TOO_DEEP = "mrd exceeds the mrd the reference orbit was computed for"
# (what differs from a served call, the message); orbit mrd 100, view 16 x 16 of span 1e-10, pixel (3, 4), mrd 50
DEEP_REFUSALS = [
    (dict(orbit=None), "orbit is NULL"),
    (dict(view=None), "view is NULL"),
    (dict(width=0), "empty view"),
    (dict(height=0), "empty view"),
    (dict(ncols=0), "empty window"),
    (dict(nrows=0), "empty window"),
    (dict(col0=10, ncols=7), "window exceeds the view"),
    (dict(row0=16, nrows=1), "window exceeds the view"),
    (dict(width=1 << 16, height=1 << 16, ncols=1 << 16, nrows=(1 << 15) + 1), "window larger than 2^31 pixels"),
    (dict(range_r=2.0 ** -961), RANGE),
    (dict(range_i=4.5), RANGE),
    (dict(range_r=float("nan")), RANGE),
    (dict(range_i=float("inf")), RANGE),
    (dict(mrd=101), TOO_DEEP),
    (dict(col=16), "pixel outside the view"),
    (dict(row=16), "pixel outside the view"),
    # two faults at once: the one reported
    (dict(orbit=None, range_r=float("nan")), "orbit is NULL"),
    (dict(width=0, mrd=101), "empty view"),
]


@pytest.mark.parametrize("change, message", DEEP_REFUSALS, ids=[",".join(c) for c, _ in DEEP_REFUSALS])
def test_validator_refusals_status_and_message(change, message):
    from distributedmandelbrot_amd import DeepOrbit
    from distributedmandelbrot_amd.device import _error_text
    L, lib = _lib()
    orbit = DeepOrbit("0", "1", 100, min_span=1e-10)
    f = dict(dict(range_r=1e-10, range_i=1e-10, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16), **change)
    cv = L.mbk_deep_view(*[f[k] for k in ("range_r", "range_i", "width", "height", "col0", "row0", "ncols", "nrows")])
    h = orbit._h if "orbit" not in change else None
    pv = C.byref(cv) if "view" not in change else None
    cc, mm, ss = C.c_int32(-7), C.c_double(-7.0), C.c_uint64(7)
    st = lib.mbk_deep_bla_count_host(h, pv, f.get("col", 3), f.get("row", 4), f.get("mrd", 50), C.byref(cc), C.byref(mm), C.byref(ss))
    assert (st, _error_text(lib)) == (L.MBK_ERR_INVALID, message)
    assert (cc.value, mm.value, ss.value) == (-7, -7.0, 7)
    if message not in (TOO_DEEP, "pixel outside the view"):      # mbk_deep_bla_info runs the same validator and takes no pixel
        levels, entries = C.c_uint32(9), C.c_uint64(9)
        st = lib.mbk_deep_bla_info(h, pv, C.byref(levels), C.byref(entries))
        assert (st, _error_text(lib)) == (L.MBK_ERR_INVALID, message)
        assert (levels.value, entries.value) == (9, 9)
