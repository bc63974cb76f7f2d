"""Extended-range deep views on the GPU (include/mbk.h, "Extended-range deep views"): the kernel is held bit for bit to the
numpy restatement of the contract (tests/deep_wide_model.py) on the library's own wide orbit table, through every entry
point.  The views are small (24 x 20 and below): each test takes seconds, most of it the model."""
import ctypes as C

import numpy as np
import pytest

import deep_model as D
import deep_wide_model as W
import histogram_model as H
import render_model as R
import smooth_truth as T
from distributedmandelbrot_amd import DeepOrbit, MbkError, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import equalize_lut

pytestmark = pytest.mark.gpu

I = ("0", "1")
TINY = ("1e-400", "0")
# (centre, range, exp2, mrd, precision_bits (None: the default for the span), at least this many distinct counts)
MAIN = {
    "i-1100": (I, 1.0, -1100, 1000, None, 8),
    "i-3000": (I, 1.0, -3000, 2500, None, 8),
    "1e-400": (TINY, 4.0, 0, 300, 1408, 8),     # every Z_m at a return to 0 is ~2^-1328: read from the wide table alone
}

_orbits, _models = {}, {}


def _orbit(centre, mrd, bits, exp2):
    key = (centre, mrd, bits, exp2)
    if key not in _orbits:
        _orbits[key] = (DeepOrbit(*centre, mrd, precision_bits=bits) if bits
                        else DeepOrbit(*centre, mrd, min_span_exp2=exp2 - 1))
    return _orbits[key]


def _model(orbit, view, mrd, window=None):
    """(counts, mag) of the window under the model, [nrows, ncols]; computed once per (orbit, view, mrd, window), read-only."""
    key = (id(orbit), view, mrd, window)
    if key not in _models:
        dr, di = W.offsets(view, window)
        c, mag = W.model_counts(*orbit.wide_table(), dr, di, view.exp2, mrd)
        rows = window[3] if window else view.height
        c, mag = c.reshape(rows, -1), mag.reshape(rows, -1)
        c.setflags(write=False)
        mag.setflags(write=False)
        _models[key] = (c, mag, orbit)      # (the orbit is kept alive with its id)
    return _models[key][:2]


def _case(name, size=(24, 20)):
    centre, rng, exp2, mrd, bits, distinct = MAIN[name]
    return _orbit(centre, mrd, bits, exp2), WideDeepView(rng, exp2, *size), mrd, distinct


def _bytes(counts, mrd):
    """ceil(count * 256 / mrd) mod 256 in exact integers."""
    return ((counts.astype(np.int64) * 256 + mrd - 1) // mrd % 256).astype(np.uint8)


def _smooth_against_truth(sm, mc, mag, what):
    """The tolerance rule of tests/test_gpu_deep.py: nu against the truth at (model count, model mag) within
    A ulp(nu) + B 2^-52, and against numpy's evaluation by the sum of the two bounds."""
    T.assert_pair(sm, D.smooth_from(mc, mag), mc, what)
    T.assert_within(sm, mc, mag, what)


def _check(gpu, orbit, view, mrd, window=None, smooth=True):
    """compute_deep_view against the model: counts, bytes, smooth (its inputs are the count and mag), statistics."""
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=mrd > 0, want_smooth=smooth)
    mc, mag = _model(orbit, view, mrd, window)
    assert np.array_equal(c, mc), (mrd, window, int((c != mc).sum()))
    if mrd > 0:
        assert np.array_equal(b, _bytes(mc, mrd)), (mrd, window)
    if smooth:
        assert (sm[mc == 0] == 0.0).all()
        _smooth_against_truth(sm, mc, mag, f"wide exp2 {view.exp2} mrd {mrd} window {window}")
    assert st.pixel_iterations == int(np.where(mc > 0, mc, max(mrd - 1, 0)).astype(np.int64).sum()), mrd
    assert st.never_pixels == int((mc == 0).sum())
    return c


@pytest.mark.parametrize("name", list(MAIN))
def test_counts_bytes_smooth_equal_the_model(gpu, name):
    """24 x 20: three columns of blocks, the last rows of blocks partial."""
    orbit, view, mrd, distinct = _case(name)
    c = _check(gpu, orbit, view, mrd)
    assert len(np.unique(c)) >= distinct
    if name == "1e-400":
        zr, zi = orbit.table()
        assert not zr.any() and not zi.any() and (c == 0).any() and (c > 0).any()
    else:
        assert (c > 0).all()


def test_window_equals_the_whole_view(gpu):
    orbit, view, mrd, _ = _case("i-1100")
    whole = _check(gpu, orbit, view, mrd, smooth=False)
    window = (5, 3, 9, 7)
    part = _check(gpu, orbit, view, mrd, window)
    assert np.array_equal(part, whole[3:10, 5:14]) and len(np.unique(part)) >= 4


@pytest.mark.parametrize("size", [(1, 1), (1, 17), (17, 1)], ids=["1x1", "1x17", "17x1"])
def test_degenerate_shapes(gpu, size):
    orbit, _, mrd, _ = _case("i-1100")
    view = WideDeepView(1.0, -1100, *size)
    c = _check(gpu, orbit, view, mrd)
    assert c.shape == size[::-1]
    if size == (1, 1):
        assert c[0, 0] == 0           # dc = 0: the pixel is the centre i itself, which never escapes


@pytest.mark.parametrize("mrd", [0, 1, 2])
def test_smallest_mrd(gpu, mrd):
    """mrd 0 and 1 run no step (every count 0); mrd 2 runs one, after which no pixel this deep has escaped."""
    orbit, view, _, _ = _case("i-1100")
    c = _check(gpu, orbit, view, mrd)
    assert not c.any()
    if mrd == 0:
        with pytest.raises(MbkError):
            gpu.compute_deep_view(orbit, view, 0, want_bytes=True)


def test_one_step_orbit(gpu):
    """Centre -2: M = 1, the start state is rebased and so is every step.  Against the model only: the tip of the antenna is a
    known limit of the contract against the truth (tests/test_deep_truth.py)."""
    mrd, exp2 = 400, -1100
    orbit = _orbit(("-2", "0"), mrd, None, exp2)
    assert orbit.length == 1 and orbit.escaped
    _check(gpu, orbit, WideDeepView(1.0, exp2, 24, 20), mrd)


def test_launch_compute_and_submit_agree(gpu):
    import torch
    from distributedmandelbrot_amd.sharding import render_deep_view
    orbit, view, mrd, _ = _case("1e-400")
    mc, _ = _model(orbit, view, mrd)
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, want_smooth=True)
    assert np.array_equal(c, mc) and np.array_equal(b, _bytes(mc, mrd))
    assert st.pixel_iterations == int(np.where(mc > 0, mc, mrd - 1).astype(np.int64).sum())
    assert st.never_pixels == int((mc == 0).sum()) > 0
    # submit / wait, two slots at once
    oc = [np.empty((10, 24), np.int32) for _ in range(2)]
    ob = [np.empty((10, 24), np.uint8) for _ in range(2)]
    for s in range(2):
        gpu.submit_deep_view(s, orbit, view, mrd, window=(0, 10 * s, 24, 10), out_counts=oc[s], out_bytes=ob[s])
    stats = [gpu.wait(s) for s in range(2)]
    assert np.array_equal(np.vstack(oc), c) and np.array_equal(np.vstack(ob), b)
    assert sum(s.pixel_iterations for s in stats) == st.pixel_iterations
    assert sum(s.never_pixels for s in stats) == st.never_pixels
    # device pointers on a caller's stream, with guards around the outputs
    n = 20 * 24
    stream = torch.cuda.Stream()
    dc = torch.full((n + 16,), -5, dtype=torch.int32, device="cuda:0")
    db = torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda:0")
    ds = torch.full((n + 16,), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.data_ptr() + 32, d_bytes=db.data_ptr() + 8, d_smooth=ds.data_ptr() + 64,
                             stream=stream.cuda_stream)
    stream.synchronize()
    gc, gb, gs = dc.cpu().numpy(), db.cpu().numpy(), ds.cpu().numpy()
    assert np.array_equal(gc[8:8 + n].reshape(20, 24), c) and (gc[:8] == -5).all() and (gc[8 + n:] == -5).all()
    assert np.array_equal(gb[8:8 + n].reshape(20, 24), b) and (gb[:8] == 7).all() and (gb[8 + n:] == 7).all()
    assert np.array_equal(gs[8:8 + n].reshape(20, 24), sm) and (gs[:8] == -1.0).all() and (gs[8 + n:] == -1.0).all()
    # row bands over the devices of this process
    rc, rb, per = render_deep_view([gpu], orbit, view, mrd, band_rows=8)
    assert np.array_equal(rc, c) and np.array_equal(rb, b) and per[0]["bands"] == 3
    with pytest.raises(ValueError):
        render_deep_view([gpu], orbit, view, mrd, bla=True)


RENDER_PAL = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255))
BYTES_PAL = Palette(np.random.RandomState(8).randint(0, 256, (256, 4)).astype(np.uint8), inside=(9, 8, 7, 255))
EQ_PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255)).for_equalized()


@pytest.mark.parametrize("source", ["bytes", "smooth", "equalized"])
@pytest.mark.parametrize("s", [1, 2])
def test_render_equals_the_render_model_on_the_models_samples(gpu, source, s):
    """A 16 x 12 image of the centre-1e-400 view (escaped and never-escaped pixels, counts 0 .. 34).  The samples are the
    model's counts, their exact bytes, and nu as the device computes it from the model's count and mag (held to the model
    by the tolerance rule here, since nu is not bit-reproducible in numpy)."""
    centre, rng, exp2, mrd, bits, _ = MAIN["1e-400"]
    orbit = _orbit(centre, mrd, bits, exp2)
    w, h = 16, 12
    view = WideDeepView(rng, exp2, w, h)
    finer = WideDeepView(rng, exp2, w * s, h * s, view.range_i)
    mc, mag = _model(orbit, finer, mrd)
    counts, _, nu, st_s = gpu.compute_deep_view(orbit, finer, mrd, want_bytes=False, want_smooth=True)
    assert np.array_equal(counts, mc) and len(np.unique(mc)) >= 8
    _smooth_against_truth(nu, mc, mag, f"wide render samples s {s}")
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
        img, st = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    if source == "equalized":           # lut=None takes the whole view's histogram on the device: the same table
        img, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s)
        assert np.array_equal(img, want)
    part, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source=source, supersample=s, window=(3, 2, 9, 7), **kw)
    assert np.array_equal(part, want[2:9, 3:12])
    import torch
    buf = torch.full((64 + want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_deep_view(orbit, view, mrd, palette=pal, d_rgba=buf.data_ptr() + 64, source=source, supersample=s, **kw)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[64:64 + want.size].reshape(want.shape), want)
    assert (got[:64] == 0xA5).all() and (got[64 + want.size:] == 0xA5).all()


@pytest.mark.parametrize("name", ["i-1100", "1e-400"])
def test_histogram_equals_bincount_of_the_models_counts(gpu, name):
    import torch
    orbit, view, mrd, _ = _case(name)
    mc, _ = _model(orbit, view, mrd)
    hist, st = gpu.deep_view_histogram(orbit, view, mrd, want_stats=True)
    assert hist.dtype == np.uint64 and np.array_equal(hist, np.bincount(mc.ravel(), minlength=mrd).astype(np.uint64))
    assert st.never_pixels == int(hist[0])
    assert st.pixel_iterations == int(np.where(mc > 0, mc, mrd - 1).astype(np.int64).sum())
    part = gpu.deep_view_histogram(orbit, view, mrd, window=(5, 3, 9, 7))
    assert np.array_equal(part, np.bincount(mc[3:10, 5:14].ravel(), minlength=mrd).astype(np.uint64))
    d = torch.zeros(mrd, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_deep_view_histogram(orbit, view, mrd, d_hist=d.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().astype(np.uint64), hist)


def test_two_orbits_keep_their_own_wide_copies(gpu):
    """Two orbits with different pictures (the second centre lies four view widths from the first and escapes), used
    alternately on one ctx, one of them also through the plain kernel (the binary64 copy and the wide copy of an orbit live
    side by side)."""
    from distributedmandelbrot_amd import DeepView
    mrd, exp2 = 1000, -1100
    a = _orbit(I, mrd, None, exp2)
    b = _orbit(("3e-331", "1"), mrd, None, exp2)
    view = WideDeepView(1.0, exp2, 24, 20)
    ma, mb = _model(a, view, mrd)[0], _model(b, view, mrd)[0]
    assert a.length == mrd and b.escaped and not np.array_equal(ma, mb)
    plain = DeepView(1e-30, 24, 20)
    pa = D.model_counts(*a.table(), *D.offsets(plain), mrd)[0].reshape(20, 24)
    for orbit, want in ((a, ma), (b, mb), (a, ma), (b, mb)):
        c, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
        assert np.array_equal(c, want)
        if orbit is a:
            c, _, _, _ = gpu.compute_deep_view(a, plain, mrd, want_bytes=False)
            assert np.array_equal(c, pa)
    out = [np.empty((20, 24), np.int32) for _ in range(2)]
    gpu.submit_deep_view(0, a, view, mrd, out_counts=out[0])
    gpu.submit_deep_view(1, b, view, mrd, out_counts=out[1])
    gpu.wait(0)
    gpu.wait(1)
    assert np.array_equal(out[0], ma) and np.array_equal(out[1], mb)


def test_refusals_write_nothing(gpu):
    lib, st = gpu._lib, L.mbk_stats()
    orbit, view, mrd, _ = _case("1e-400")
    n = 20 * 24
    oc, ob, osm = np.full(n, -7, np.int32), np.full(n, 7, np.uint8), np.full(n, -7.0)
    both = L.MBK_WANT_COUNTS | L.MBK_WANT_BYTES

    def xview(**kw):
        f = dict(range_r=4.0, range_i=4.0, exp2=0, width=24, height=20, col0=0, row0=0, ncols=24, nrows=20)
        f.update(kw)
        return L.mbk_deep_xview(*[f[k] for k in ("range_r", "range_i", "exp2", "width", "height", "col0", "row0", "ncols", "nrows")])

    def compute(cv, m=mrd, flags=both, orb=orbit):
        return lib.mbk_deep_xview_compute(gpu._h, orb._h if orb is not None else None, C.byref(cv), m, flags, oc.ctypes.data,
                                          ob.ctypes.data, osm.ctypes.data, C.byref(st))

    bad_views = [xview(range_r=2.0 ** -65), xview(range_i=4.5), xview(range_r=float("nan")), xview(exp2=1), xview(exp2=-8193),
                 xview(ncols=0), xview(nrows=0), xview(col0=20, ncols=5), xview(row0=20, nrows=1),
                 xview(width=1 << 16, height=1 << 16, ncols=1 << 16, nrows=(1 << 15) + 1)]
    for cv in bad_views:
        assert compute(cv) == L.MBK_ERR_INVALID
        assert lib.mbk_deep_xview_submit(gpu._h, 1, orbit._h, C.byref(cv), mrd, both, oc.ctypes.data, ob.ctypes.data) == L.MBK_ERR_INVALID
    ok = xview()
    assert compute(ok, m=mrd + 1) == L.MBK_ERR_INVALID                       # beyond the orbit's mrd
    assert compute(ok, orb=None) == L.MBK_ERR_INVALID
    for flags in (both | L.MBK_DEEP_BLA, both | L.MBK_KERNEL_GROUP, both | L.MBK_PRECISION_F32, both | L.MBK_LAZY_UNIFORM):
        assert compute(ok, flags=flags) == L.MBK_ERR_INVALID, flags
        assert lib.mbk_deep_xview_launch(gpu._h, orbit._h, C.byref(ok), mrd, flags, None, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_submit(gpu._h, 7, orbit._h, C.byref(ok), mrd, both, oc.ctypes.data, ob.ctypes.data) == L.MBK_ERR_INVALID
    assert (oc == -7).all() and (ob == 7).all() and (osm == -7.0).all()
    # renders: the distance sources and every flag; histograms: every flag
    img = np.full((20, 24, 4), 0xA5, np.uint8)
    for source in ("distance", "distance_rel"):
        spec = Palette.cosine(64).spec(source, 1, 0)
        assert lib.mbk_deep_xview_render_compute(gpu._h, orbit._h, C.byref(ok), mrd, 0, C.byref(spec), img.ctypes.data,
                                                 C.byref(st)) == L.MBK_ERR_INVALID, source
    spec = RENDER_PAL.spec("smooth", 1, 0)
    hist = np.full(mrd, 7, np.uint64)
    for flags in (L.MBK_DEEP_BLA, L.MBK_KERNEL_SCAN):
        assert lib.mbk_deep_xview_render_compute(gpu._h, orbit._h, C.byref(ok), mrd, flags, C.byref(spec), img.ctypes.data,
                                                 C.byref(st)) == L.MBK_ERR_INVALID
        assert lib.mbk_deep_xview_histogram_compute(gpu._h, orbit._h, C.byref(ok), mrd, flags, hist.ctypes.data,
                                                    C.byref(st)) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_render_compute(gpu._h, orbit._h, C.byref(xview(exp2=1)), mrd, 0, C.byref(spec), img.ctypes.data,
                                             C.byref(st)) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_histogram_compute(gpu._h, orbit._h, C.byref(xview(range_r=5.0)), mrd, 0, hist.ctypes.data,
                                                C.byref(st)) == L.MBK_ERR_INVALID
    assert (img == 0xA5).all() and (hist == 7).all()
    # the Python methods refuse what a wide view does not have before they call the library
    with pytest.raises(ValueError):
        gpu.compute_deep_view(orbit, view, mrd, bla=True)
    with pytest.raises(ValueError):
        gpu.deep_view_histogram(orbit, view, mrd, bla=True)
    with pytest.raises(ValueError):
        gpu.render_deep_view(orbit, view, mrd, palette=RENDER_PAL, source="distance_rel")
    with pytest.raises(ValueError):
        gpu.compute_deep_view_distance(orbit, view, mrd)
    # the ctx still works afterwards
    c, _, _, _ = gpu.compute_deep_view(orbit, view, mrd)
    assert np.array_equal(c, _model(orbit, view, mrd)[0])
