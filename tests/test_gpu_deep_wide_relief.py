"""Relief shading for extended-range deep views on the GPU (include/mbk.h, the section of that name), held to the numpy model
of the contract (tests/deep_wide_relief_model.py).

The normals involve no libm call, so the device must store the model's value on every pixel and bit, with the plain wide step
and with the skips of MBK_DEEP_XBLA.  The other outputs of the one pass are held to the calls whose bits they are: the counts
to compute_deep_view(xbla=...), nu to its smooth values, rel to compute_wide_view_distance / _distance_xbla (device against
device: no logarithm stands between them).  A relief render is mbk_relief_resolve_host (held to the numpy rule by
tests/test_relief.py and tests/test_deep_wide_relief.py) of the device's own samples of the s times finer view -- with the
table of that view -- banded or not, whole or windowed.  Views are 24 x 20 at exp2 -1100 and at 1e-400, 16 x 12 at exp2 -3000,
the sizes of tests/test_gpu_deep_wide_distance_bla.py, and the ragged 61 x 45.
"""
import ctypes as C
import math

import numpy as np
import pytest

import deep_wide_relief_model as WR
import relief_model as RM
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, MbkError, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _cxview, _error_text
from distributedmandelbrot_amd.image import relief_resolve_host
from test_deep_wide import MIS, TINY

pytestmark = pytest.mark.gpu

# name -> (centre, range, exp2, mrd, precision_bits (None: the default for the span), width, height)
CASES = {
    "i-1100": (("0", "1"), 1.0, -1100, 3000, None, 24, 20),
    "mis-3000": (MIS, 1.0, -3000, 9000, None, 16, 12),
    "1e-400": (TINY, 4.0, 0, 300, 1408, 24, 20),
    "i-3000": (("0", "1"), 1.0, -3000, 6000, None, 16, 12),     # the longest orbit: ~60 skips per pixel stand for 6000 steps
}
WHOLE = ("i-1100", "mis-3000", "1e-400")
RULES = [False, True]            # xbla
RAGGED = (3, 5, 13, 11)          # a window at an odd offset whose sides are no multiples of 8
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _orbit(name):
    if name not in _cache:
        centre, rng, exp2, mrd, bits, w, h = CASES[name]
        view = WideDeepView(rng, exp2, w, h)
        orbit = DeepOrbit(*centre, mrd, precision_bits=bits) if bits else DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)
        _cache[name] = (orbit, view, mrd)
    return _cache[name]


def _model(name, xbla):
    """The model of the case's whole view: computed once, shared, left unchanged."""
    if ("model", name, xbla) not in _cache:
        orbit, view, mrd = _orbit(name)
        _cache["model", name, xbla] = WR.model(orbit, view, mrd, xbla=xbla)
    return _cache["model", name, xbla]


def _distance(gpu, orbit, view, mrd, xbla, window=None):
    return (gpu.compute_wide_view_distance_xbla if xbla else gpu.compute_wide_view_distance)(orbit, view, mrd, window=window)


def _check(gpu, orbit, view, mrd, xbla, model, what, window=None):
    """Every output of the one pass against what it is defined to equal; returns (counts, normals)."""
    want, mn, _, _, st = model
    counts, normals, nu, rel, stats = gpu.compute_wide_view_normals(orbit, view, mrd, window=window, xbla=xbla, want_smooth=True,
                                                                    want_distance=True)
    assert counts.dtype == np.int32 and normals.dtype == np.float64 and normals.shape == counts.shape + (2,)
    ref, _, smooth, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, want_smooth=True, xbla=xbla)
    drel, dcounts, _ = _distance(gpu, orbit, view, mrd, xbla, window)
    assert np.array_equal(counts, ref) and np.array_equal(counts, dcounts) and np.array_equal(counts, mn), (what, int((counts != mn).sum()))
    assert _same_bits(normals, want), (what, int((_bits(normals) != _bits(want)).any(axis=2).sum()))
    assert _same_bits(nu, smooth), what
    assert _same_bits(rel, drel), what
    assert not np.isnan(normals).any(), what
    assert np.array_equal((normals == 0.0).all(axis=2), counts == 0), what          # flat exactly where nothing escaped
    assert not np.signbit(normals[counts == 0]).any(), what
    lit = normals[counts > 0]
    assert (np.abs(np.hypot(lit[:, 0], lit[:, 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all(), what
    iters = np.where(counts > 0, counts, max(mrd - 1, 0)).astype(np.int64).sum()
    assert stats.pixel_iterations == int(iters) and stats.never_pixels == int((counts == 0).sum()), what
    # without the optional outputs: the same normals and counts
    c2, n2, _ = gpu.compute_wide_view_normals(orbit, view, mrd, window=window, xbla=xbla)
    assert np.array_equal(c2, counts) and _same_bits(n2, normals), what
    return counts, normals


def _whole(gpu, name, xbla):
    if ("whole", name, xbla) not in _cache:
        orbit, view, mrd = _orbit(name)
        counts, normals = _check(gpu, orbit, view, mrd, xbla, _model(name, xbla), (name, xbla))
        counts.setflags(write=False)
        normals.setflags(write=False)
        _cache["whole", name, xbla] = (counts, normals)
    return _cache["whole", name, xbla]


@pytest.mark.parametrize("xbla", RULES)
@pytest.mark.parametrize("name", WHOLE)
def test_whole_views_every_pixel_and_bit(gpu, name, xbla):
    orbit, view, mrd = _orbit(name)
    counts, normals = _whole(gpu, name, xbla)
    st = _model(name, xbla)[4]
    esc = st["n"] > 0
    assert esc.mean() >= 0.8 and len(np.unique(counts)) >= 5
    if name == "1e-400":            # every step adds an orbit entry binary64 cannot hold (2^-1328); no level is ever taken
        assert (st["xmin"][esc] < -1022).all() and np.array_equal(st["steps"], np.where(esc, st["n"], mrd - 1))
    else:                           # |d| ~ 1 / (distance to the set): far above binary64, and it drops out all the same
        assert (st["e"][esc] > -view.exp2).all()
        if xbla:
            assert st["steps"].sum() < 0.5 * np.where(esc, st["n"], mrd - 1).sum()


def test_the_longest_orbit_on_the_device(gpu):
    """c = i at 2^-3000, mrd 6000, 16 x 12: every pixel takes tens of skips over several levels in place of thousands of steps.
    Normals equal the model and none is flat."""
    orbit, view, mrd = _orbit("i-3000")
    model = _model("i-3000", True)
    counts, normals = _check(gpu, orbit, view, mrd, True, model, "i-3000")
    st = model[4]
    esc = st["n"] > 0
    assert esc.mean() > 0.9 and (counts[counts > 0] > 2000).all() and (st["steps"][esc] < 0.1 * st["n"][esc]).all()
    _check(gpu, orbit, view, mrd, False, _model("i-3000", False), "i-3000 plain")


@pytest.mark.parametrize("xbla", RULES)
def test_ragged_and_thin_views_and_windows(gpu, xbla):
    orbit, view, mrd = _orbit("i-1100")
    # 61 x 45: partial 8x8 blocks on both edges; a single row; a single column.  The counts of these views lie in 881 .. 916:
    # mrd 885 (887 for the column) leaves about a quarter (a sixth) of the pixels without a count
    for thin, shallow in ((WideDeepView(1.0, -1100, 61, 45), 885), (WideDeepView(1.0, -1100, 64, 1, 1.0), 885),
                          (WideDeepView(1.0, -1100, 1, 33, 1.0), 887)):
        model = WR.model(orbit, thin, shallow, xbla=xbla)
        assert 0.1 < (model[1] == 0).mean() < 0.5, (model[1] == 0).mean()
        _check(gpu, orbit, thin, shallow, xbla, model, (thin.width, thin.height, xbla))
    wc, whole = _whole(gpu, "i-1100", xbla)
    for window in (RAGGED, (23, 19, 1, 1), (0, 8, 24, 8), (5, 0, 3, 20)):
        c0, r0, nc, nr = window
        counts, normals, nu, rel, st = gpu.compute_wide_view_normals(orbit, view, mrd, window=window, xbla=xbla, want_smooth=True,
                                                                     want_distance=True)
        assert np.array_equal(counts, wc[r0:r0 + nr, c0:c0 + nc]) and _same_bits(normals, whole[r0:r0 + nr, c0:c0 + nc]), window
        assert _same_bits(rel, _distance(gpu, orbit, view, mrd, xbla, window)[0])
        assert _same_bits(nu, gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, want_smooth=True, xbla=xbla)[2])
        assert st.pixel_iterations == int(np.where(counts > 0, counts, mrd - 1).astype(np.int64).sum())
    ragged = WideDeepView(1.0, -1100, 29, 23)
    _check(gpu, orbit, ragged, 885, xbla, WR.model(orbit, ragged, 885, window=RAGGED, xbla=xbla), "ragged window", window=RAGGED)


def test_no_skip_identity_on_the_device(gpu):
    """An orbit of length 1 (no table: the plain kernel whatever the flag) and a view whose offsets never pass level 0's radius
    (the xbla kernel, plain side only): bit for bit the plain rule."""
    m1 = DeepOrbit("-2", "0", 400, min_span_exp2=-1100)
    assert m1.length == 1
    tiny, tview, tmrd = _orbit("1e-400")
    assert tiny.length >= 2
    for orbit, view, mrd in ((m1, WideDeepView(1.0, -1100, 24, 20), 400), (m1, WideDeepView(1.0, -1100, 29, 23), 400), (tiny, tview, tmrd)):
        a = gpu.compute_wide_view_normals(orbit, view, mrd, xbla=True, want_smooth=True, want_distance=True)
        b = gpu.compute_wide_view_normals(orbit, view, mrd, xbla=False, want_smooth=True, want_distance=True)
        assert np.array_equal(a[0], b[0]) and (a[0] > 0).any()
        for x, y in zip(a[1:4], b[1:4]):
            assert _same_bits(x, y)
        want, mn, _, _, st = WR.model(orbit, view, mrd, xbla=True)
        assert np.array_equal(st["steps"], np.where(st["n"] > 0, st["n"], mrd - 1))          # no skip was taken
        assert np.array_equal(a[0], mn) and _same_bits(a[1], want)


@pytest.mark.parametrize("xbla", RULES)
def test_shallow_mrd(gpu, xbla):
    far = DeepOrbit("0", "1", 10, precision_bits=128)            # a view wide enough that pixels escape at the first steps
    assert far.length >= 2                                        # (so there is a table)
    view = WideDeepView(4.0, 0, 24, 20)
    for mrd in (0, 1, 2, 5):
        for window in (None, RAGGED):
            counts, normals, nu, rel, st = gpu.compute_wide_view_normals(far, view, mrd, window=window, xbla=xbla, want_smooth=True,
                                                                         want_distance=True)
            want, mn, _, _, _ = WR.model(far, view, mrd, window, xbla=xbla)
            assert np.array_equal(counts, mn) and _same_bits(normals, want)
            if mrd < 2:
                assert not counts.any() and not normals.any() and not nu.any() and not rel.any()
                assert st.pixel_iterations == 0 and st.never_pixels == counts.size
    assert mn.max() > 0 and (mn == 0).any() and (want[mn > 0] != 0.0).any(axis=1).all()
    # no pixel of a deep view escapes at step 1: mrd 2 stores zeros
    orbit, deep, _ = _orbit("i-1100")
    counts, normals, nu, rel, _ = gpu.compute_wide_view_normals(orbit, deep, 2, xbla=xbla, want_smooth=True, want_distance=True)
    assert not counts.any() and not normals.any() and not nu.any() and not rel.any()


def test_launch_on_a_torch_stream_with_guards(gpu):
    """Into sentinel-filled buffers with guard rows in front of and behind the window, for each combination of NULL optional
    outputs: every element of the window is written, flat normals included, and nothing outside it."""
    import torch
    orbit, view, _ = _orbit("i-1100")
    mrd = 887                   # about a tenth of the pixels never escape: their flat normals, zero nu and zero rel are written too
    guard = 3 * 24
    stream = torch.cuda.Stream(device="cuda:0")
    for xbla in RULES:
        model = WR.model(orbit, view, mrd, xbla=xbla)
        assert 0.02 < (model[1] == 0).mean() < 0.5
        wc, whole = _check(gpu, orbit, view, mrd, xbla, model, ("launch", xbla))
        for window in (None, RAGGED):
            c0, r0, nc, nr = window or (0, 0, view.width, view.height)
            want, want_c = whole[r0:r0 + nr, c0:c0 + nc], wc[r0:r0 + nr, c0:c0 + nc]
            px = want_c.size
            _, _, nu, rel, _ = gpu.compute_wide_view_normals(orbit, view, mrd, window=window, xbla=xbla, want_smooth=True, want_distance=True)
            forms = [(wc_, ws, wr) for wc_ in (True, False) for ws in (True, False) for wr in (True, False)]
            bufs = [(torch.full((2 * (px + 2 * guard),), -77.0, dtype=torch.float64, device="cuda:0"),
                     torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0"),
                     torch.full((px + 2 * guard,), -78.0, dtype=torch.float64, device="cuda:0"),
                     torch.full((px + 2 * guard,), -79.0, dtype=torch.float64, device="cuda:0")) for _ in forms]
            torch.cuda.synchronize()
            for (dn, dc, ds, dr), (with_c, with_s, with_r) in zip(bufs, forms):
                gpu.launch_wide_view_normals(orbit, view, mrd, d_normals=dn[2 * guard:].data_ptr(),
                                             d_counts=dc[guard:].data_ptr() if with_c else 0,
                                             d_smooth=ds[guard:].data_ptr() if with_s else 0,
                                             d_rel=dr[guard:].data_ptr() if with_r else 0, stream=stream.cuda_stream, window=window, xbla=xbla)
            stream.synchronize()
            for (dn, dc, ds, dr), form in zip(bufs, forms):
                hn, hc, hs, hr = (t.cpu().numpy() for t in (dn, dc, ds, dr))
                assert _same_bits(hn[2 * guard:2 * (guard + px)].reshape(want.shape), want), (xbla, window, form)
                assert (hn[:2 * guard] == -77.0).all() and (hn[2 * (guard + px):] == -77.0).all(), (xbla, window, form)
                for h, sentinel, given, ref in ((hc, -5, form[0], want_c), (hs, -78.0, form[1], nu), (hr, -79.0, form[2], rel)):
                    assert (h[:guard] == sentinel).all() and (h[guard + px:] == sentinel).all(), (xbla, window, form)
                    if given:
                        got = h[guard:guard + px].reshape(ref.shape)
                        assert np.array_equal(got, ref) if ref.dtype == np.int32 else _same_bits(got, ref), (xbla, window, form)
                    else:
                        assert (h == sentinel).all(), (xbla, window, form)


def _render_palette():
    rng = np.random.RandomState(11)
    return Palette(rng.randint(0, 256, (53, 4)).astype(np.uint8), inside=(9, 8, 7, 200), scale=3.7, offset=0.25)


@pytest.mark.parametrize("xbla", RULES)
@pytest.mark.parametrize("s", [1, 2, 3])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s, xbla):
    """The sample view at s x is a full view of its own: with xbla its samples are made with its own table."""
    orbit, mrd = _orbit("i-1100")[0], 887          # (about a tenth of the samples never escape)
    w, h = 40, 28
    view = WideDeepView(1.0, -1100, w, h)
    fine = WideDeepView(1.0, -1100, w * s, h * s, view.range_i)
    pal = _render_palette()
    counts, normals, nu, st_s = gpu.compute_wide_view_normals(orbit, fine, mrd, xbla=xbla, want_smooth=True)
    assert 0.03 < (counts == 0).mean() < 0.3 and len(np.unique(counts)) > 5
    light, height = (math.cos(0.6), math.sin(0.6)), 1.25
    want = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=normals, light=light, height=height)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    inside = (counts.reshape(h, s, w, s) == 0).all(axis=(1, 3))
    assert inside.any() and (want[inside] == np.array(pal.inside, np.uint8)).all()         # the inside colour is unshaded
    for rows in (0, 3):
        img, st = gpu.render_wide_view_relief(orbit, view, mrd, palette=pal, light=light, height=height, supersample=s, xbla=xbla,
                                              max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (7, 5, 19, 13)
    img, _ = gpu.render_wide_view_relief(orbit, view, mrd, palette=pal, light=light, height=height, supersample=s, xbla=xbla, window=window,
                                         max_band_rows=4)
    assert np.array_equal(img, want[5:18, 7:26])
    # the launch form on a caller's stream, guard words behind the image
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_wide_view_relief(orbit, view, mrd, palette=pal, d_rgba=d.data_ptr(), light=light, height=height, supersample=s,
                                       xbla=xbla, stream=stream.cuda_stream, max_band_rows=5)
    stream.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


@pytest.mark.parametrize("xbla", RULES)
def test_the_neutral_shade(gpu, xbla):
    """height 2^10 without a light: every escaped sample takes the neutral q = 255 -- the smooth image scaled by 255 / 256 --
    and the inside colour none."""
    orbit, mrd = _orbit("i-1100")[0], 887
    view = WideDeepView(1.0, -1100, 40, 28)
    pal = _render_palette()
    flat, _ = gpu.render_wide_view_relief(orbit, view, mrd, palette=pal, light=(0.0, 0.0), height=2.0 ** 10, xbla=xbla)
    smooth, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source="smooth", xbla=xbla)
    counts, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False, xbla=xbla)
    assert RM.neutral(2.0 ** 10) == 255
    want = smooth.astype(np.int64)
    want[..., :3] = (want[..., :3] * 255 + 128) >> 8
    want[counts == 0] = pal.inside
    assert np.array_equal(flat, want) and (counts == 0).any() and (counts > 0).any()
    lit, _ = gpu.render_wide_view_relief(orbit, view, mrd, palette=pal, xbla=xbla)                 # 45 degrees, height 1.5
    assert (lit != flat).any(axis=2).sum() > 200


def test_the_table_is_shared_with_the_count_and_distance_launches(gpu):
    """A count launch with xbla=True, a distance launch and a normal launch in turn on one orbit: first on one set of spans (one
    table, built once by whichever comes first), then on two.  Every result equals that of a fresh context."""
    orbit, view, mrd = _orbit("i-1100")
    views = (view, WideDeepView(1.0, -1090, 24, 20))
    want = {}
    with MandelbrotDevice(0) as fresh:
        for k, v in enumerate(views):
            want[k] = fresh.compute_wide_view_normals(orbit, v, mrd, xbla=True, want_smooth=True, want_distance=True)[:4]
    assert not np.array_equal(want[0][0], want[1][0])
    assert np.array_equal(want[0][0], _model("i-1100", True)[1]) and _same_bits(want[0][1], _model("i-1100", True)[0])

    def turn(k, order):
        for what in order:
            if what == "count":
                c, _, nu, _ = gpu.compute_deep_view(orbit, views[k], mrd, want_bytes=False, want_smooth=True, xbla=True)
                assert np.array_equal(c, want[k][0]) and _same_bits(nu, want[k][2]), (k, what)
            elif what == "distance":
                rel, c, _ = gpu.compute_wide_view_distance_xbla(orbit, views[k], mrd)
                assert np.array_equal(c, want[k][0]) and _same_bits(rel, want[k][3]), (k, what)
            else:
                got = gpu.compute_wide_view_normals(orbit, views[k], mrd, xbla=True, want_smooth=True, want_distance=True)
                assert np.array_equal(got[0], want[k][0]) and all(_same_bits(a, b) for a, b in zip(got[1:4], want[k][1:])), (k, what)

    for order in (("count", "distance", "normal"), ("normal", "count", "distance")):      # one set of spans
        turn(0, order)
    for k in (0, 1, 0, 1, 1):                                                             # two
        turn(k, ("count", "distance", "normal"))
    for k in (1, 0):
        turn(k, ("normal", "distance", "count"))


def test_refusals_write_nothing(gpu):
    """Argument checks that return before any launch: status, message, nothing written, and the ctx works afterwards."""
    import torch
    lib = gpu._lib
    orbit = DeepOrbit("0", "1", 500, min_span_exp2=-1100)
    view = WideDeepView(1.0, -1100, 16, 16)
    cv = _cxview(view)
    guard = 64
    dn = torch.full((2 * (256 + 2 * guard),), -77.0, dtype=torch.float64, device="cuda:0")
    dd = torch.full((256 + 2 * guard,), -78.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((256 + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    di = torch.full((256 + 2 * guard,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pn, pd, pc, pi = dn[2 * guard:].data_ptr(), dd[guard:].data_ptr(), dc[guard:].data_ptr(), di[guard:].data_ptr()
    launch, compute = lib.mbk_deep_xview_launch_normal, lib.mbk_deep_xview_compute_normal
    rl, rc = lib.mbk_deep_xview_relief_render_launch, lib.mbk_deep_xview_relief_render_compute
    hn, h, hc, himg = np.full(512, -1.0), np.full(256, -2.0), np.full(256, -9, np.int32), np.full((16, 16, 4), 3, np.uint8)
    pal = _render_palette()
    spec = pal.relief_spec(1)
    both = (0, L.MBK_DEEP_XBLA)

    def refused(st, message=None):
        assert st == L.MBK_ERR_INVALID
        if message is not None:
            assert _error_text(lib, gpu._h) == message

    def four(message, bad=cv, mrd=100, flags=0, orb=orbit._h, renders=True):
        """the four device calls on valid buffers"""
        view_p = C.byref(bad) if bad is not None else None
        refused(launch(gpu._h, orb, view_p, mrd, flags, pc, pn, pd, pd, None), message)
        refused(compute(gpu._h, orb, view_p, mrd, flags, hc.ctypes.data, hn.ctypes.data, h.ctypes.data, h.ctypes.data, None), message)
        if renders:
            refused(rl(gpu._h, orb, view_p, mrd, flags, C.byref(spec), pi, None), message)
            refused(rc(gpu._h, orb, view_p, mrd, flags, C.byref(spec), himg.ctypes.data, None), message)

    # a NULL normal, spec, palette or output pointer; a misaligned d_normal or d_rgba
    for flags in both:
        refused(launch(gpu._h, orbit._h, C.byref(cv), 100, flags, pc, None, pd, pd, None), "NULL normal pointer")
        refused(compute(gpu._h, orbit._h, C.byref(cv), 100, flags, hc.ctypes.data, None, h.ctypes.data, h.ctypes.data, None), "NULL normal pointer")
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, None, pi, None), "render spec is NULL")
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, None, himg.ctypes.data, None), "render spec is NULL")
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), None, None), "output pointer is NULL")
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), None, None), "output pointer is NULL")
        refused(launch(gpu._h, orbit._h, C.byref(cv), 100, flags, pc, pn + 4, pd, pd, None), "d_normal must be 8-byte aligned")
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), pi + 2, None), "d_rgba must be 4-byte aligned")
    with pytest.raises(MbkError):
        gpu.launch_wide_view_normals(orbit, view, 100, d_normals=0, d_counts=pc)
    no_palette = pal.relief_spec(1)
    no_palette.palette = None
    bad_specs = [no_palette, pal.relief_spec(5), pal.relief_spec(1, light=(1.5, 0.0)), pal.relief_spec(1, light=(0.0, math.nan)),
                 pal.relief_spec(1, height=-0.5), pal.relief_spec(1, height=2.0 ** 10 + 1), pal.relief_spec(1, height=math.nan),
                 Palette(pal.entries[:1]).relief_spec(1), Palette(pal.entries, scale=0.0).relief_spec(1)]
    for bad in bad_specs:
        for flags in both:
            refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(bad), pi, None))
            refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(bad), himg.ctypes.data, None))
    # MBK_DEEP_BLA in the count calls' words; every other flag with a text of these calls' own
    for flags in (L.MBK_DEEP_BLA, L.MBK_DEEP_BLA | L.MBK_DEEP_XBLA, L.MBK_DEEP_BLA | L.MBK_WANT_COUNTS):
        four("MBK_DEEP_BLA is not implemented for extended-range deep views", flags=flags)
    for flags in (L.KERNELS["asm"], L.KERNELS["scan"], L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_WANT_COUNTS, L.MBK_WANT_BYTES,
                  L.MBK_DEEP_XBLA | L.MBK_WANT_COUNTS, 0x80000000):
        four("extended-range deep normals take MBK_DEEP_XBLA only (no kernel selection, no fp32)", flags=flags)
    # every refusal of tests/test_gpu_deep_wide_distance_bla.py's table of views
    views = [(dict(range_r=2.0 ** -65), "extended-range deep view ranges must be finite and lie in [2^-64, 4]"),
             (dict(range_i=4.5), "extended-range deep view ranges must be finite and lie in [2^-64, 4]"),
             (dict(range_r=float("nan")), "extended-range deep view ranges must be finite and lie in [2^-64, 4]"),
             (dict(exp2=1), "extended-range deep view exp2 must lie in [-8192, 0]"),
             (dict(exp2=-8193), "extended-range deep view exp2 must lie in [-8192, 0]"),
             (dict(width=0), "empty view"), (dict(ncols=0), "empty window"), (dict(col0=10, ncols=7), "window exceeds the view"),
             (dict(mrd=501), "mrd exceeds the mrd the reference orbit was computed for")]
    ok = dict(range_r=1.0, range_i=1.0, exp2=-1100, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16)
    for change, text in views:
        f = dict(ok, **change)
        bad = L.mbk_deep_xview(*[f[k] for k in ("range_r", "range_i", "exp2", "width", "height", "col0", "row0", "ncols", "nrows")])
        for flags in both:
            four(text, bad=bad, mrd=f.get("mrd", 100), flags=flags, renders="width" not in change)      # (a render of an empty view
            #                                                                       is refused for its geometry first)
    for flags in both:
        four("orbit is NULL", orb=None, flags=flags)
        four("view is NULL", bad=None, flags=flags)
    refused(launch(None, orbit._h, C.byref(cv), 100, 0, pc, pn, pd, pd, None))
    refused(rc(None, orbit._h, C.byref(cv), 100, 0, C.byref(spec), himg.ctypes.data, None))
    with pytest.raises(MbkError):
        gpu.compute_wide_view_normals(orbit, view, 501)
    with pytest.raises(MbkError):
        gpu.render_wide_view_relief(orbit, view, 100, palette=pal, height=-1.0)
    with pytest.raises(MbkError):
        gpu.render_wide_view_relief(orbit, view, 100, palette=pal, window=(10, 0, 7, 16), xbla=True)

    # each family names the other: a DeepView here is a ValueError, a WideDeepView there the deep calls' MbkError
    plain = DeepView(1e-20, 16, 16)
    for call in (lambda v: gpu.compute_wide_view_normals(orbit, v, 100), lambda v: gpu.launch_wide_view_normals(orbit, v, 100, d_normals=pn),
                 lambda v: gpu.render_wide_view_relief(orbit, v, 100, palette=pal),
                 lambda v: gpu.launch_render_wide_view_relief(orbit, v, 100, palette=pal, d_rgba=pi)):
        with pytest.raises(ValueError, match="takes a WideDeepView"):
            call(plain)
    for call in (lambda: gpu.compute_deep_view_normals(orbit, view, 100),
                 lambda: gpu.launch_deep_view_normals(orbit, view, 100, d_normals=pn, d_counts=pc),
                 lambda: gpu.render_deep_view_relief(orbit, view, 100, palette=pal),
                 lambda: gpu.launch_render_deep_view_relief(orbit, view, 100, palette=pal, d_rgba=pi)):
        with pytest.raises(MbkError, match="DeepView only.*2\\^-960"):
            call()

    torch.cuda.synchronize()
    assert (dn.cpu().numpy() == -77.0).all() and (dd.cpu().numpy() == -78.0).all() and (dc.cpu().numpy() == -5).all()
    assert (di.cpu().numpy() == -3).all() and (hn == -1.0).all() and (h == -2.0).all() and (hc == -9).all() and (himg == 3).all()
    # the ctx serves a call afterwards
    for xbla in RULES:
        counts, normals, _ = gpu.compute_wide_view_normals(orbit, view, 100, xbla=xbla)
        want, mn, _, _, _ = WR.model(orbit, view, 100, xbla=xbla)
        assert np.array_equal(counts, mn) and _same_bits(normals, want)
        img, _ = gpu.render_wide_view_relief(orbit, view, 100, palette=pal, xbla=xbla)
        assert img.shape == (16, 16, 4)
