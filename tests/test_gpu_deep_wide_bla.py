"""Extended-range deep views with bilinear approximation on the GPU (include/mbk.h, "Extended-range deep views with bilinear
approximation"): deep_wide_bla_kernel is held bit for bit to the numpy restatement of the contract
(tests/deep_wide_bla_model.py) on the library's own wide orbit table, through every entry point that takes MBK_DEEP_XBLA.
The views are small (24 x 20 and below): each test takes seconds, most of it the model."""
import ctypes as C

import numpy as np
import pytest

import deep_model as D
import deep_wide_bla_model as X
import deep_wide_model as W
import histogram_model as H
import render_model as R
import smooth_truth as T
from test_deep_wide import MIS, TINY
from distributedmandelbrot_amd import DeepOrbit, DeepView, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import equalize_lut

pytestmark = pytest.mark.gpu

I = ("0", "1")
# (centre, range, exp2, mrd, precision_bits (None: the default for the span), at least this many distinct counts)
MAIN = {
    "i-1100": (I, 1.0, -1100, 3000, None, 8),
    "mis-1100": (MIS, 1.0, -1100, 4000, None, 8),
    "1e-400": (TINY, 4.0, 0, 300, 1408, 8),     # span 4 against |Z| ~ 2^-1328: the table is there and no pixel may use it
}

_orbits, _models = {}, {}


def _orbit(centre, mrd, bits, exp2):
    key = (centre, mrd, bits, exp2)
    if key not in _orbits:
        _orbits[key] = (DeepOrbit(*centre, mrd, precision_bits=bits) if bits
                        else DeepOrbit(*centre, mrd, min_span_exp2=exp2 - 2))
    return _orbits[key]


def _model(orbit, view, mrd, window=None, xbla=True):
    """(counts, mag, steps) of the window under the model (xbla False: the non-BLA wide model, steps None), [nrows, ncols];
    computed once per key, read-only.  The table is the full view's."""
    key = (id(orbit), view, mrd, window, xbla)
    if key not in _models:
        dr, di = W.offsets(view, window)
        tab = orbit.wide_table()
        if xbla:
            out = X.counts(*tab, dr, di, view.exp2, mrd, X.build(*tab, X.dcmax(view)))
        else:
            out = W.model_counts(*tab, dr, di, view.exp2, mrd) + (None,)
        rows = window[3] if window else view.height
        out = tuple(a.reshape(rows, -1) if a is not None else None for a in out)
        for a in out[:2]:
            a.setflags(write=False)
        _models[key] = out + (orbit,)      # (the orbit is kept alive with its id)
    return _models[key][:3]


def _case(name, size=(24, 20)):
    centre, rng, exp2, mrd, bits, distinct = MAIN[name]
    return _orbit(centre, mrd, bits, exp2), WideDeepView(rng, exp2, *size), mrd, distinct


def _bytes(counts, mrd):
    """ceil(count * 256 / mrd) mod 256 in exact integers."""
    return ((counts.astype(np.int64) * 256 + mrd - 1) // mrd % 256).astype(np.uint8)


def _smooth_against_truth(sm, mc, mag, what):
    """The tolerance rule of tests/test_gpu_deep_wide.py: nu against the truth at (model count, model mag) within
    A ulp(nu) + B 2^-52, and against numpy's evaluation by the sum of the two bounds."""
    T.assert_pair(sm, D.smooth_from(mc, mag), mc, what)
    T.assert_within(sm, mc, mag, what)


def _check(gpu, orbit, view, mrd, window=None, smooth=True):
    """compute_deep_view(xbla=True) against the model: counts, bytes, smooth (its inputs are the count and mag), statistics
    (the reference's iterations, not the steps executed)."""
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=mrd > 0, want_smooth=smooth, xbla=True)
    mc, mag, _ = _model(orbit, view, mrd, window)
    assert np.array_equal(c, mc), (mrd, window, int((c != mc).sum()))
    if mrd > 0:
        assert np.array_equal(b, _bytes(mc, mrd)), (mrd, window)
    if smooth:
        assert (sm[mc == 0] == 0.0).all()
        _smooth_against_truth(sm, mc, mag, f"xbla exp2 {view.exp2} mrd {mrd} window {window}")
    assert st.pixel_iterations == int(np.where(mc > 0, mc, max(mrd - 1, 0)).astype(np.int64).sum()), mrd
    assert st.never_pixels == int((mc == 0).sum())
    return c


@pytest.mark.parametrize("name", list(MAIN))
def test_counts_bytes_smooth_equal_the_model(gpu, name):
    """24 x 20: three columns of blocks, the last rows of blocks partial."""
    orbit, view, mrd, distinct = _case(name)
    c = _check(gpu, orbit, view, mrd)
    assert len(np.unique(c)) >= distinct
    steps = _model(orbit, view, mrd)[2]
    plain = int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
    if name == "1e-400":
        assert int(steps.sum()) == plain and (c == 0).any() and (c > 0).any()
        assert np.array_equal(c, _model(orbit, view, mrd, xbla=False)[0])
    else:
        assert (c > 0).all() and 10 * int(steps.sum()) < plain                       # the model these counts equal did skip


def test_launch_compute_and_submit_agree(gpu):
    import torch
    orbit, view, mrd, _ = _case("i-1100")
    other, _, omrd, _ = _case("mis-1100")
    mc, mag, _ = _model(orbit, view, mrd)
    oc_model = _model(other, view, omrd)[0]
    assert not np.array_equal(mc, oc_model)
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, want_smooth=True, xbla=True)
    assert np.array_equal(c, mc) and np.array_equal(b, _bytes(mc, mrd))
    # submit / wait, two slots at once, two orbits (each with its own table)
    oc = [np.empty((20, 24), np.int32) for _ in range(2)]
    ob = [np.empty((20, 24), np.uint8) for _ in range(2)]
    gpu.submit_deep_view(0, orbit, view, mrd, out_counts=oc[0], out_bytes=ob[0], xbla=True)
    gpu.submit_deep_view(1, other, view, omrd, out_counts=oc[1], out_bytes=ob[1], xbla=True)
    stats = [gpu.wait(s) for s in range(2)]
    assert np.array_equal(oc[0], mc) and np.array_equal(ob[0], b)
    assert np.array_equal(oc[1], oc_model) and np.array_equal(ob[1], _bytes(oc_model, omrd))
    assert stats[0].pixel_iterations == st.pixel_iterations == int(mc.astype(np.int64).sum())
    assert stats[1].pixel_iterations == int(oc_model.astype(np.int64).sum()) and stats[1].never_pixels == 0
    # device pointers on a caller's stream, with guards around the outputs
    n = 20 * 24
    stream = torch.cuda.Stream()
    dc = torch.full((n + 16,), -5, dtype=torch.int32, device="cuda:0")
    db = torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda:0")
    ds = torch.full((n + 16,), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.data_ptr() + 32, d_bytes=db.data_ptr() + 8, d_smooth=ds.data_ptr() + 64,
                             stream=stream.cuda_stream, xbla=True)
    stream.synchronize()
    gc, gb, gs = dc.cpu().numpy(), db.cpu().numpy(), ds.cpu().numpy()
    assert np.array_equal(gc[8:8 + n].reshape(20, 24), c) and (gc[:8] == -5).all() and (gc[8 + n:] == -5).all()
    assert np.array_equal(gb[8:8 + n].reshape(20, 24), b) and (gb[:8] == 7).all() and (gb[8 + n:] == 7).all()
    assert np.array_equal(gs[8:8 + n].reshape(20, 24), sm) and (gs[:8] == -1.0).all() and (gs[8 + n:] == -1.0).all()


@pytest.mark.parametrize("centre, M", [(("-2", "0"), 1), (("1.5", "0"), 2), (("0.9", "0"), 3)], ids=["M1", "M2", "M3"])
def test_smallest_orbits(gpu, centre, M):
    """M = 1: no table, the flag changes nothing.  M = 2 and 3: tables of one entry and of two."""
    mrd, exp2 = 400, -1100
    orbit = _orbit(centre, mrd, None, exp2)
    assert orbit.length == M and orbit.escaped
    view = WideDeepView(1.0, exp2, 24, 20)
    c = _check(gpu, orbit, view, mrd)
    if M == 1:
        assert np.array_equal(c, _model(orbit, view, mrd, xbla=False)[0])


@pytest.mark.parametrize("size", [(9, 1), (1, 1), (1, 9)], ids=["9x1", "1x1", "1x9"])
def test_degenerate_shapes(gpu, size):
    """A single row or column holds the zero-dcm pixel; the 1 x 1 view has dcmax 0 as well."""
    orbit, _, mrd, _ = _case("i-1100")
    c = _check(gpu, orbit, WideDeepView(1.0, -1100, *size), mrd)
    assert c.shape == size[::-1] and c[size[1] // 2, size[0] // 2] == 0          # dc = 0: the centre i, which never escapes
    if size != (1, 1):
        assert (np.delete(c.ravel(), c.size // 2) > 0).all()


def test_window_and_bands_equal_the_whole_view(gpu):
    from distributedmandelbrot_amd.sharding import render_deep_view
    orbit, view, mrd, _ = _case("i-1100")
    whole = _check(gpu, orbit, view, mrd, smooth=False)
    window = (5, 3, 9, 7)
    part = _check(gpu, orbit, view, mrd, window)
    assert np.array_equal(part, whole[3:10, 5:14]) and len(np.unique(part)) >= 4
    rc, rb, per = render_deep_view([gpu], orbit, view, mrd, band_rows=8, xbla=True)
    assert np.array_equal(rc, whole) and np.array_equal(rb, _bytes(whole, mrd)) and per[0]["bands"] == 3
    with pytest.raises(ValueError):
        render_deep_view([gpu], orbit, view, mrd, bla=True)
    with pytest.raises(ValueError):
        render_deep_view([gpu], orbit, view, mrd, bla=True, xbla=True)


def test_launch_mrd_below_the_orbits(gpu):
    """i + 2^l <= mrd: launches that end on a skip boundary (257: steps 1 .. 256 are one skip of level 8), one past it, and at
    and just past a pixel's count (tests/test_deep_wide_bla.py scans 40 such values on the host twin)."""
    orbit, view, mrd, _ = _case("i-1100")
    full = _model(orbit, view, mrd)[0]
    n = int(np.sort(full.ravel())[full.size // 2])
    for m in (257, 258, n, n + 1):
        c = _check(gpu, orbit, view, m, smooth=False)
        assert (c < m).all() and np.array_equal(c, np.where(full < m, full, 0))
    assert (_model(orbit, view, 257)[2] == 1).all() and (_model(orbit, view, 258)[2] == 2).all()


def test_the_cached_table_is_replaced_not_reused(gpu):
    """One orbit, one ctx, spans alternating: the same dcmax mantissa under another exp2, then another mantissa; the non-BLA
    wide kernel on the same orbit in between."""
    mrd = 3000
    orbit = _orbit(I, mrd, None, -1102)
    a, b, c = WideDeepView(1.0, -1100, 24, 20), WideDeepView(1.0, -1101, 24, 20), WideDeepView(1.5, -1100, 24, 20)
    assert X.dcmax(a)[0] == X.dcmax(b)[0] != X.dcmax(c)[0] and X.dcmax(a)[1] == X.dcmax(b)[1] + 1
    models = {v: _model(orbit, v, mrd)[0] for v in (a, b, c)}
    assert not np.array_equal(models[a], models[b]) and not np.array_equal(models[a], models[c])
    for v in (a, b, a, c, b, c, a):
        got, _, _, _ = gpu.compute_deep_view(orbit, v, mrd, want_bytes=False, xbla=True)
        assert np.array_equal(got, models[v]), v
        if v is a:
            got, _, _, _ = gpu.compute_deep_view(orbit, a, mrd, want_bytes=False)
            assert np.array_equal(got, _model(orbit, a, mrd, xbla=False)[0])


RENDER_PAL = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255))
BYTES_PAL = Palette(np.random.RandomState(8).randint(0, 256, (256, 4)).astype(np.uint8), inside=(9, 8, 7, 255))
EQ_PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255)).for_equalized()


@pytest.mark.parametrize("source", ["bytes", "smooth", "equalized"])
@pytest.mark.parametrize("s", [1, 2])
def test_render_equals_the_render_model_on_the_models_samples(gpu, source, s):
    """A 16 x 12 image of the centre-1e-400 view, as tests/test_gpu_deep_wide.py renders it, with xbla: the samples are the
    model's counts at s times the width and height (a full view of its own, with its own dcmax), their exact bytes, and nu
    as the device computes it from the model's count and mag."""
    centre, rng, exp2, mrd, bits, _ = MAIN["1e-400"]
    orbit = _orbit(centre, mrd, bits, exp2)
    w, h = 16, 12
    view = WideDeepView(rng, exp2, w, h)
    finer = WideDeepView(rng, exp2, w * s, h * s, view.range_i)
    mc, mag, _ = _model(orbit, finer, mrd)
    counts, _, nu, st_s = gpu.compute_deep_view(orbit, finer, mrd, want_bytes=False, want_smooth=True, xbla=True)
    assert np.array_equal(counts, mc) and len(np.unique(mc)) >= 8
    _smooth_against_truth(nu, mc, mag, f"xbla render samples s {s}")
    if source == "bytes":
        pal = BYTES_PAL
        want = R.render_bytes(pal.entries, s, _bytes(mc, mrd))
        kw = {}
    elif source == "smooth":
        pal = RENDER_PAL
        want = R.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, s, mc, nu)
        kw = {}
    else:
        pal = EQ_PAL
        hist = np.bincount(_model(orbit, view, mrd)[0].ravel(), minlength=mrd).astype(np.uint64)   # at OUTPUT resolution
        table = equalize_lut(hist)
        want = H.render_equalized(pal.entries, pal.inside, pal.scale, pal.offset, table, s, mc, nu)
        kw = {"lut": table}
    assert len(np.unique(want.reshape(-1, 4), axis=0)) >= 8
    for rows in (0, 5):
        img, st = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s, max_band_rows=rows, xbla=True)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    if source == "equalized":           # lut=None takes the whole view's histogram on the device, with xbla: the same table
        img, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s, xbla=True)
        assert np.array_equal(img, want)
    part, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s, window=(3, 2, 9, 7), xbla=True, **kw)
    assert np.array_equal(part, want[2:9, 3:12])
    import torch
    buf = torch.full((64 + want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_deep_view(orbit, view, mrd, palette=pal, d_rgba=buf.data_ptr() + 64, source=source, supersample=s, xbla=True, **kw)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:64 + want.size].reshape(want.shape), want)
    assert (got[:64] == 0xA5).all() and (got[64 + want.size:] == 0xA5).all()


def test_render_of_a_view_that_skips(gpu):
    """The same three sources at s = 2 on a 12 x 8 image of the i-1100 view, whose samples do take skips."""
    orbit, _, mrd, _ = _case("i-1100")
    view = WideDeepView(1.0, -1100, 12, 8)
    finer = WideDeepView(1.0, -1100, 24, 16, view.range_i)
    mc, mag, steps = _model(orbit, finer, mrd)
    assert 10 * int(steps.sum()) < int(mc.astype(np.int64).sum())
    _, _, nu, _ = gpu.compute_deep_view(orbit, finer, mrd, want_bytes=False, want_smooth=True, xbla=True)
    _smooth_against_truth(nu, mc, mag, "xbla render samples of i-1100")
    table = equalize_lut(np.bincount(_model(orbit, view, mrd)[0].ravel(), minlength=mrd).astype(np.uint64))
    wants = {"bytes": (BYTES_PAL, R.render_bytes(BYTES_PAL.entries, 2, _bytes(mc, mrd))),
             "smooth": (RENDER_PAL, R.render_smooth(RENDER_PAL.entries, RENDER_PAL.inside, RENDER_PAL.scale, RENDER_PAL.offset, 2, mc, nu)),
             "equalized": (EQ_PAL, H.render_equalized(EQ_PAL.entries, EQ_PAL.inside, EQ_PAL.scale, EQ_PAL.offset, table, 2, mc, nu))}
    for source, (pal, want) in wants.items():
        img, st = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=2, xbla=True)
        assert np.array_equal(img, want), source
        assert st.pixel_iterations == int(mc.astype(np.int64).sum()) and st.never_pixels == 0


@pytest.mark.parametrize("name", ["i-1100", "1e-400"])
def test_histogram_equals_bincount_of_the_models_counts(gpu, name):
    import torch
    orbit, view, mrd, _ = _case(name)
    mc = _model(orbit, view, mrd)[0]
    hist, st = gpu.deep_view_histogram(orbit, view, mrd, want_stats=True, xbla=True)
    assert hist.dtype == np.uint64 and np.array_equal(hist, np.bincount(mc.ravel(), minlength=mrd).astype(np.uint64))
    assert st.never_pixels == int(hist[0])
    assert st.pixel_iterations == int(np.where(mc > 0, mc, mrd - 1).astype(np.int64).sum())
    part = gpu.deep_view_histogram(orbit, view, mrd, window=(5, 3, 9, 7), xbla=True)
    assert np.array_equal(part, np.bincount(mc[3:10, 5:14].ravel(), minlength=mrd).astype(np.uint64))
    d = torch.zeros(mrd, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_deep_view_histogram(orbit, view, mrd, d_hist=d.data_ptr(), xbla=True)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint64), hist)


def test_refusals_write_nothing(gpu):
    from distributedmandelbrot_amd.device import _error_text
    lib, st = gpu._lib, L.mbk_stats()
    orbit, view, mrd, _ = _case("1e-400")
    n = 20 * 24
    oc, ob, osm = np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, -7.0)
    both, XBLA, BLA = L.MBK_WANT_COUNTS | L.MBK_WANT_BYTES, L.MBK_DEEP_XBLA, L.MBK_DEEP_BLA
    p = (oc.ctypes.data, ob.ctypes.data)
    xv = L.mbk_deep_xview(4.0, 4.0, 0, 24, 20, 0, 0, 24, 20)
    dv = L.mbk_deep_view(1e-10, 1e-10, 24, 20, 0, 0, 24, 20)
    pv = L.mbk_view(-2.0, -2.0, 4.0, 4.0, 24, 20, 0, 0, 24, 20)
    plain_orbit = _orbit(I, 100, 128, 0)
    calls = [
        lambda f: lib.mbk_deep_view_compute(gpu._h, plain_orbit._h, C.byref(dv), 100, both | f, *p, osm.ctypes.data, C.byref(st)),
        lambda f: lib.mbk_deep_view_submit(gpu._h, 1, plain_orbit._h, C.byref(dv), 100, both | f, *p),
        lambda f: lib.mbk_view_compute(gpu._h, C.byref(pv), 100, both | f, *p, C.byref(st)),
        lambda f: lib.mbk_view_launch(gpu._h, C.byref(pv), 100, both | f, None, None, None),
        lambda f: lib.mbk_julia_view_compute(gpu._h, C.byref(pv), 0.3, 0.5, 100, both | f, *p, osm.ctypes.data, C.byref(st)),
        lambda f: lib.mbk_deep_view_compute_distance(gpu._h, plain_orbit._h, C.byref(dv), 100, f, oc.ctypes.data, osm.ctypes.data, C.byref(st)),
        lambda f: lib.mbk_deep_view_launch_distance(gpu._h, plain_orbit._h, C.byref(dv), 100, f, None, None, None),
        lambda f: lib.mbk_view_compute_distance(gpu._h, C.byref(pv), 100, f, oc.ctypes.data, osm.ctypes.data, C.byref(st)),
    ]
    for k, call in enumerate(calls):
        assert call(XBLA) == L.MBK_ERR_INVALID, k
    # both flags at once, on every form of the count call: MBK_DEEP_BLA's own refusal, verbatim
    for flags in (both | XBLA | BLA, both | BLA):
        assert lib.mbk_deep_xview_compute(gpu._h, orbit._h, C.byref(xv), mrd, flags, *p, osm.ctypes.data, C.byref(st)) == L.MBK_ERR_INVALID
        assert _error_text(lib, gpu._h) == "MBK_DEEP_BLA is not implemented for extended-range deep views"
        assert lib.mbk_deep_xview_submit(gpu._h, 1, orbit._h, C.byref(xv), mrd, flags, *p) == L.MBK_ERR_INVALID
        assert lib.mbk_deep_xview_launch(gpu._h, orbit._h, C.byref(xv), mrd, flags, None, None, None, None) == L.MBK_ERR_INVALID
    for flags in (both | XBLA | L.MBK_KERNEL_GROUP, both | XBLA | L.MBK_PRECISION_F32):
        assert lib.mbk_deep_xview_compute(gpu._h, orbit._h, C.byref(xv), mrd, flags, *p, osm.ctypes.data, C.byref(st)) == L.MBK_ERR_INVALID
    assert (oc == -7).all() and (ob == 7).all() and (osm == -7.0).all()
    # renders: the distance sources stay refused with the flag, and so does the flag beside another; histograms likewise
    img = np.full((20, 24, 4), 0xA5, np.uint8)
    for source in ("distance", "distance_rel"):
        spec = Palette.cosine(64).spec(source, 1, 0)
        assert lib.mbk_deep_xview_render_compute(gpu._h, orbit._h, C.byref(xv), mrd, XBLA, C.byref(spec), img.ctypes.data,
                                                 C.byref(st)) == L.MBK_ERR_INVALID, source
        assert _error_text(lib, gpu._h) == "distance estimates are not implemented for extended-range deep views"
    spec = RENDER_PAL.spec("smooth", 1, 0)
    hist = np.full(mrd, 7, np.uint64)
    for flags in (XBLA | BLA, XBLA | L.MBK_KERNEL_SCAN):
        assert lib.mbk_deep_xview_render_compute(gpu._h, orbit._h, C.byref(xv), mrd, flags, C.byref(spec), img.ctypes.data,
                                                 C.byref(st)) == L.MBK_ERR_INVALID
        assert lib.mbk_deep_xview_histogram_compute(gpu._h, orbit._h, C.byref(xv), mrd, flags, hist.ctypes.data,
                                                    C.byref(st)) == L.MBK_ERR_INVALID
    dspec = RENDER_PAL.spec("smooth", 1, 0)
    assert lib.mbk_deep_view_render_compute(gpu._h, plain_orbit._h, C.byref(dv), 100, XBLA, C.byref(dspec), img.ctypes.data,
                                            C.byref(st)) == L.MBK_ERR_INVALID
    assert lib.mbk_view_render_compute(gpu._h, C.byref(pv), 100, XBLA, C.byref(dspec), img.ctypes.data, C.byref(st)) == L.MBK_ERR_INVALID
    assert lib.mbk_view_histogram_compute(gpu._h, C.byref(pv), 100, XBLA, hist.ctypes.data, C.byref(st)) == L.MBK_ERR_INVALID
    assert (img == 0xA5).all() and (hist == 7).all()
    # the Python methods: xbla is the wide view's, bla the plain view's, and never both
    plain = DeepView(1e-10, 24, 20)
    with pytest.raises(ValueError, match="bla=True"):
        gpu.compute_deep_view(plain_orbit, plain, 100, xbla=True)
    with pytest.raises(ValueError):
        gpu.compute_deep_view(plain_orbit, plain, 100, bla=True, xbla=True)
    with pytest.raises(ValueError):
        gpu.deep_view_histogram(plain_orbit, plain, 100, xbla=True)
    with pytest.raises(ValueError):
        gpu.render_deep_view(plain_orbit, plain, 100, palette=RENDER_PAL, xbla=True)
    with pytest.raises(ValueError):
        gpu.compute_deep_view(orbit, view, mrd, bla=True)
    with pytest.raises(ValueError):
        gpu.compute_deep_view(orbit, view, mrd, bla=True, xbla=True)
    with pytest.raises(ValueError):
        gpu.render_deep_view(orbit, view, mrd, palette=RENDER_PAL, source="distance_rel", xbla=True)
    # the ctx still works afterwards
    c, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, xbla=True)
    assert np.array_equal(c, _model(orbit, view, mrd)[0])
