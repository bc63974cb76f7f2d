"""Deep-zoom views with bilinear approximation on the GPU (include/mbk.h, "Deep-zoom views with bilinear approximation"):
the kernel is held bit for bit to the numpy restatement of the contract (tests/deep_bla_model.py) on the library's own
orbit table, through every entry point that takes MBK_DEEP_BLA; the calls that do not take it refuse it."""
import functools

import numpy as np
import pytest

import deep_bla_model as B
import deep_model as D
import smooth_truth as T
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, View
from distributedmandelbrot_amd.image import Palette, resolve_host

pytestmark = pytest.mark.gpu

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
# (centre, span, view, mrd, at least this many distinct counts, skips: the model executes at most half the plain rule's steps)
CASES = [
    (SEAHORSE, 1e-20, (128, 96), 30000, 20, True),
    (("0", "1"), 1e-200, (64, 64), 5000, 20, True),
    (("1e-21", "1"), 1e-20, (100, 70), 5000, 20, False),   # M = 58: a skip may end on m == M, and the pixel rebases there
    (("-2", "0"), 1e-60, (40, 24), 200, 1, False),          # M = 1: no table, the flag changes nothing
    (("0", "1"), 1e-30, (13, 9), 3000, 8, True),            # partial blocks
]


@functools.lru_cache(maxsize=None)
def _orbit(centre, mrd, span):
    return DeepOrbit(*centre, mrd, min_span=span)


@functools.lru_cache(maxsize=None)
def _model(centre, span, size, mrd, launch_mrd=None, window=None, span_i=None, orbit_span=None):
    """(orbit, view, counts, mag, steps) of the BLA model, computed once per case."""
    orbit = _orbit(centre, mrd, span if orbit_span is None else orbit_span)
    view = DeepView(span, *size, span_i)
    zr, zi = orbit.table()
    dr, di = D.offsets(view, window)
    table = B.build(zr, zi, B.dcmax(view))
    c, mag, steps = B.counts(zr, zi, dr, di, mrd if launch_mrd is None else launch_mrd, table)
    rows = window[3] if window else view.height
    for a in (c, mag, steps):
        a.setflags(write=False)
    return orbit, view, c.reshape(rows, -1), mag.reshape(rows, -1), steps.reshape(rows, -1)


def _bytes(counts, mrd):
    return ((counts.astype(np.int64) * 256 + mrd - 1) // mrd % 256).astype(np.uint8)


def _smooth_against_truth(sm, mc, mag, what, sample=4000):
    """As tests/test_gpu_deep.py: nu at (model count, model mag) within the allowance of tests/smooth_truth.py."""
    T.assert_pair(sm, D.smooth_from(mc, mag), mc, what)
    esc = np.flatnonzero(mc.ravel() > 0)
    if esc.size > sample:
        esc = np.random.RandomState(4).choice(esc, sample, replace=False)
    if esc.size:
        T.assert_within(sm.ravel()[esc], mc.ravel()[esc], mag.ravel()[esc], what)


def _check(gpu, orbit, view, mrd, mc, mag, window=None):
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, window=window, want_smooth=True, bla=True)
    assert np.array_equal(c, mc), (mrd, window, int((c != mc).sum()))
    assert np.array_equal(b, _bytes(mc, mrd)) and np.array_equal(b, gpu.quantise_counts(c, mrd))
    assert (sm[mc == 0] == 0.0).all()
    _smooth_against_truth(sm, mc, mag, f"deep bla mrd {mrd} window {window}")
    # the statistics follow the stored counts: the reference's iterations, not the steps executed
    assert st.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
    assert st.never_pixels == int((c == 0).sum())
    return c


@pytest.mark.parametrize("centre, span, size, mrd, distinct, skips", CASES,
                         ids=["seahorse-1e-20", "i-1e-200", "M58", "M1", "13x9"])
def test_counts_bytes_smooth_equal_the_model(gpu, centre, span, size, mrd, distinct, skips):
    orbit, view, mc, mag, steps = _model(centre, span, size, mrd)
    c = _check(gpu, orbit, view, mrd, mc, mag)
    assert len(np.unique(c)) >= distinct
    plain = int(np.where(mc > 0, mc, mrd - 1).astype(np.int64).sum())
    if skips:
        assert 2 * int(steps.sum()) <= plain, (int(steps.sum()), plain)
    if centre == ("1e-21", "1"):
        assert orbit.length == 58 and c.max() > orbit.length and int(steps.sum()) < plain
    if centre == ("-2", "0"):
        assert orbit.length == 1 and int(steps.sum()) == plain


def test_without_the_flag_the_plain_contract_holds(gpu):
    """One launch without the flag between two with it, on one orbit and view: deep_model.model_counts, bit for bit."""
    centre, span, size, mrd = ("0", "1"), 1e-30, (40, 36), 3000
    orbit, view, mc, mag, _ = _model(centre, span, size, mrd)
    _check(gpu, orbit, view, mrd, mc, mag)
    zr, zi = orbit.table()
    pc, _ = D.model_counts(zr, zi, *D.offsets(view), mrd)
    c, b, _, _ = gpu.compute_deep_view(orbit, view, mrd)
    assert np.array_equal(c.ravel(), pc) and np.array_equal(b, _bytes(c, mrd))
    _check(gpu, orbit, view, mrd, mc, mag)


@pytest.mark.parametrize("mrd", [0, 1, 2, 3, 4, 5, 9, 10, 257, 258, 1025, 1026, 1027, 3000])
def test_the_end_of_the_loop(gpu, mrd):
    """i + 2^l <= mrd: a launch's mrd on a skip boundary (2^k + 1: one skip of 2^k steps), one above it and one below it."""
    orbit, view, mc, mag, steps = _model(("0", "1"), 1e-200, (9, 7), 3000, launch_mrd=mrd)
    if mrd == 0:
        c, b, _, _ = gpu.compute_deep_view(orbit, view, 0, want_bytes=False, bla=True)
        assert b is None and not c.any()
        return
    _check(gpu, orbit, view, mrd, mc, mag)
    if 2 <= mrd <= 258:                 # nothing has escaped yet: steps 1 .. mrd-1 in as few skips as their binary form has
        assert not mc.any() and (steps == bin(mrd - 1).count("1")).all()


def test_windows_and_bands_equal_the_whole_view(gpu):
    centre, span, size, mrd = ("0", "1"), 1e-30, (100, 70), 3000
    orbit, view, mc, mag, _ = _model(centre, span, size, mrd)
    whole, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False, bla=True)
    assert np.array_equal(whole, mc) and len(np.unique(whole)) >= 20
    for window in [(0, 20, 100, 33), (13, 0, 51, 70), (99, 69, 1, 1), (64, 40, 8, 8), (3, 5, 17, 11)]:
        c0, r0, nc, nr = window
        part, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, bla=True)
        assert np.array_equal(part, whole[r0:r0 + nr, c0:c0 + nc]), window


def test_submit_torch_launch_and_bands_equal_compute(gpu):
    import torch
    from distributedmandelbrot_amd.sharding import render_deep_view
    centre, span, size, mrd = ("0", "1"), 1e-60, (120, 100), 5000
    orbit, view, mc, mag, _ = _model(centre, span, size, mrd)
    c, b, sm, _ = gpu.compute_deep_view(orbit, view, mrd, want_smooth=True, bla=True)
    assert np.array_equal(c, mc)
    oc = [np.empty((50, 120), np.int32) for _ in range(2)]
    ob = [np.empty((50, 120), np.uint8) for _ in range(2)]
    for s in range(2):
        gpu.submit_deep_view(s, orbit, view, mrd, window=(0, 50 * s, 120, 50), out_counts=oc[s], out_bytes=ob[s], bla=True)
    for s in range(2):
        gpu.wait(s)
    assert np.array_equal(np.vstack(oc), c) and np.array_equal(np.vstack(ob), b)
    stream = torch.cuda.Stream()
    dc = torch.full((100 * 120,), -5, dtype=torch.int32, device="cuda:0")
    db = torch.full((100 * 120,), 7, dtype=torch.uint8, device="cuda:0")
    ds = torch.zeros(100 * 120, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.data_ptr(), d_bytes=db.data_ptr(), d_smooth=ds.data_ptr(),
                             stream=stream.cuda_stream, bla=True)
    stream.synchronize()
    assert np.array_equal(dc.cpu().numpy().reshape(100, 120), c)
    assert np.array_equal(db.cpu().numpy().reshape(100, 120), b)
    assert np.array_equal(ds.cpu().numpy().reshape(100, 120), sm)
    rc, rb, per = render_deep_view([gpu], orbit, view, mrd, band_rows=32, bla=True)
    assert np.array_equal(rc, c) and np.array_equal(rb, b) and per[0]["bands"] == 4


def test_two_spans_in_turn_each_get_their_own_table(gpu):
    """Two views of one orbit whose spans differ, alternating on one ctx -- with two launches of different tables in flight
    on two slots at once in the middle."""
    centre, mrd = ("0", "1"), 3000
    a = _model(centre, 1e-30, (48, 40), mrd)
    b = _model(centre, 1e-12, (48, 40), mrd, orbit_span=1e-30)
    assert a[0] is b[0] and not np.array_equal(a[2], b[2])
    orbit = a[0]
    for _, view, mc, _, _ in (a, b, a, b):
        c, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False, bla=True)
        assert np.array_equal(c, mc)
    out = [np.empty((40, 48), np.int32) for _ in range(2)]
    gpu.submit_deep_view(0, orbit, a[1], mrd, out_counts=out[0], bla=True)
    gpu.submit_deep_view(1, orbit, b[1], mrd, out_counts=out[1], bla=True)
    gpu.wait(0)
    gpu.wait(1)
    assert np.array_equal(out[0], a[2]) and np.array_equal(out[1], b[2])


@pytest.mark.parametrize("source, s, mrd", [("bytes", 1, 300), ("smooth", 2, 3000)])
def test_render_equals_the_host_rule_on_the_bla_samples(gpu, source, s, mrd):
    """The counts of this view lie in 160 .. 187: the byte source runs with mrd 300, so that they quantise to more than a
    handful of bytes."""
    centre, span, orbit_mrd = ("0", "1"), 1e-60, 3000
    orbit = _orbit(centre, orbit_mrd, span)
    w, h = 61, 45
    view = DeepView(span, w, h)
    finer = DeepView(span, w * s, h * s, view.span_i)
    entries = 256 if source == "bytes" else 300             # MBK_RENDER_BYTES takes a palette of exactly 256 entries
    pal = Palette(np.random.RandomState(7).randint(0, 256, (entries, 4)).astype(np.uint8), inside=(9, 8, 7, 255))
    _, _, mc, _, _ = _model(centre, span, (w * s, h * s), orbit_mrd, launch_mrd=mrd, span_i=view.span_i)
    counts, byts, nu, st_s = gpu.compute_deep_view(orbit, finer, mrd, want_smooth=True, bla=True)
    assert np.array_equal(counts, mc) and len(np.unique(counts)) > 8
    want = resolve_host(pal, source, s, w, h, counts=counts, bytes_=byts, smooth=nu)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 8
    for rows in (0, 7):
        img, st = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s, max_band_rows=rows, bla=True)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    with pytest.raises(MbkError):
        gpu.render_deep_view(orbit, view, mrd, palette=Palette.deep_distance(view, 8.0), source="distance_rel", bla=True)


def test_histogram_equals_bincount_of_the_bla_counts(gpu):
    import torch
    centre, span, size, mrd = ("0", "1"), 1e-60, (120, 100), 5000
    orbit, view, mc, _, _ = _model(centre, span, size, mrd)
    hist, st = gpu.deep_view_histogram(orbit, view, mrd, want_stats=True, bla=True)
    assert hist.dtype == np.uint64 and np.array_equal(hist, np.bincount(mc.ravel(), minlength=mrd).astype(np.uint64))
    assert st.never_pixels == int(hist[0])
    window = (7, 9, 50, 41)
    part = gpu.deep_view_histogram(orbit, view, mrd, window=window, bla=True)
    assert np.array_equal(part, np.bincount(mc[9:50, 7:57].ravel(), minlength=mrd).astype(np.uint64))
    d = torch.zeros(mrd, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_deep_view_histogram(orbit, view, mrd, d_hist=d.data_ptr(), bla=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint64), hist)


def test_the_other_calls_refuse_the_bit(gpu):
    import ctypes as C
    from distributedmandelbrot_amd import _lib as L
    lib, st = gpu._lib, L.mbk_stats()
    out = np.empty(16 * 16, np.int32)
    val = np.empty(16 * 16, np.float64)
    cv = gpu._cview(View(-2.0, -1.5, 3.0, 3.0, 16, 16), None)
    flags = L.MBK_WANT_COUNTS | L.MBK_DEEP_BLA
    assert lib.mbk_view_compute(gpu._h, C.byref(cv), 100, flags, out.ctypes.data, None, C.byref(st)) == L.MBK_ERR_INVALID
    assert lib.mbk_julia_view_compute(gpu._h, C.byref(cv), -0.5, 0.5, 100, flags, out.ctypes.data, None, None,
                                      C.byref(st)) == L.MBK_ERR_INVALID
    orbit = _orbit(("0", "1"), 3000, 1e-30)
    dv = gpu._cdeep(DeepView(1e-30, 16), None)
    assert lib.mbk_deep_view_compute_distance(gpu._h, orbit._h, C.byref(dv), 100, L.MBK_DEEP_BLA, out.ctypes.data,
                                              val.ctypes.data, C.byref(st)) == L.MBK_ERR_INVALID
    # the deep count call still refuses everything else beside it, and the ctx works afterwards
    assert lib.mbk_deep_view_compute(gpu._h, orbit._h, C.byref(dv), 100, flags | L.MBK_KERNEL_GROUP, out.ctypes.data, None, None,
                                     C.byref(st)) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_compute(gpu._h, orbit._h, C.byref(dv), 100, flags, out.ctypes.data, None, None, C.byref(st)) == L.MBK_OK
    c, _, _ = gpu.compute_view(View(-2.0, -1.5, 3.0, 3.0, 16, 16), 100, want_bytes=False)
    assert c.shape == (16, 16)
