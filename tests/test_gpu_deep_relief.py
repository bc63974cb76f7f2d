"""Relief shading for deep views on the GPU (include/mbk.h, "Relief shading for deep views"), held to the numpy model of the
contract (tests/deep_relief_model.py).

The normals involve no libm call, so the device must store the model's value on every pixel and bit, with the plain step and with
the skips of MBK_DEEP_BLA.  The other outputs of the one pass are held to the calls whose bits they are: the counts to
compute_deep_view(bla=...), nu to its smooth values, rel to compute_deep_view_distance / _distance_bla.  A relief render is
mbk_relief_resolve_host (held to the numpy rule by tests/test_relief.py and tests/test_deep_relief.py) of the device's own
samples of the s times finer view, banded or not, whole or windowed.  Views are 64 x 64 or smaller at mrd 3000, and one 16 x 16
view at mrd 30 000 whose pixels take ~3000 skips each.
"""
import ctypes as C
import math

import numpy as np
import pytest

import deep_relief_model as RL
import relief_model as RM
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _error_text
from distributedmandelbrot_amd.image import relief_resolve_host
from test_deep_distance import CASES

pytestmark = pytest.mark.gpu

WHOLE = ("i-1e-200", "M51-1e-35", "seahorse-1e-12")
RULES = [False, True]           # bla
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _orbit(name):
    if name not in _cache:
        centre, span, mrd = CASES[name]
        _cache[name] = (DeepOrbit(*centre, mrd, min_span=span), DeepView(span, 64, 64), mrd)
    return _cache[name]


def _model(name, bla):
    """The model of the case's whole view: computed once, shared, left unchanged."""
    if ("model", name, bla) not in _cache:
        orbit, view, mrd = _orbit(name)
        _cache["model", name, bla] = RL.model(orbit, view, mrd, bla=bla)
    return _cache["model", name, bla]


def _distance(gpu, orbit, view, mrd, bla, window=None):
    return (gpu.compute_deep_view_distance_bla if bla else gpu.compute_deep_view_distance)(orbit, view, mrd, window=window)


def _check(gpu, orbit, view, mrd, bla, model, what, window=None):
    """Every output of the one pass against what it is defined to equal; returns (counts, normals)."""
    want, mn, _, _, st = model
    counts, normals, nu, rel, stats = gpu.compute_deep_view_normals(orbit, view, mrd, window=window, bla=bla, want_smooth=True,
                                                                    want_distance=True)
    assert counts.dtype == np.int32 and normals.dtype == np.float64 and normals.shape == counts.shape + (2,)
    ref, _, smooth, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, want_smooth=True, bla=bla)
    assert np.array_equal(counts, ref) and np.array_equal(counts, mn), (what, int((counts != mn).sum()))
    assert _same_bits(normals, want), (what, int((_bits(normals) != _bits(want)).any(axis=2).sum()))
    assert _same_bits(nu, smooth), what
    assert _same_bits(rel, _distance(gpu, orbit, view, mrd, bla, window)[0]), what
    assert not np.isnan(normals).any(), what
    assert np.array_equal((normals == 0.0).all(axis=2), counts == 0), what          # flat exactly where nothing escaped
    assert not np.signbit(normals[counts == 0]).any(), what
    iters = np.where(counts > 0, counts, max(mrd - 1, 0)).astype(np.int64).sum()
    assert stats.pixel_iterations == int(iters) and stats.never_pixels == int((counts == 0).sum()), what
    # without the optional outputs: the same normals and counts
    c2, n2, _ = gpu.compute_deep_view_normals(orbit, view, mrd, window=window, bla=bla)
    assert np.array_equal(c2, counts) and _same_bits(n2, normals), what
    return counts, normals


def _whole(gpu, name, bla):
    if ("whole", name, bla) not in _cache:
        orbit, view, mrd = _orbit(name)
        counts, normals = _check(gpu, orbit, view, mrd, bla, _model(name, bla), (name, bla))
        counts.setflags(write=False)
        normals.setflags(write=False)
        _cache["whole", name, bla] = (counts, normals)
    return _cache["whole", name, bla]


@pytest.mark.parametrize("bla", RULES)
@pytest.mark.parametrize("name", WHOLE)
def test_whole_views_every_pixel_and_bit(gpu, name, bla):
    orbit, view, mrd = _orbit(name)
    counts, normals = _whole(gpu, name, bla)
    st = _model(name, bla)[4]
    esc = st["n"] > 0
    assert esc.mean() >= 0.9 and len(np.unique(counts)) >= 8
    lit = normals[counts > 0]
    assert (np.abs(np.hypot(lit[:, 0], lit[:, 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
    if name == "i-1e-200":          # e past 512 on every escaped pixel: it really drops out
        assert (st["e"][esc] >= 512).all()
        if bla:
            assert st["steps"].sum() <= 0.2 * st["n"][esc].sum()
    if name == "M51-1e-35":         # the orbit wraps: rebases at m == M, lanes at different m
        assert orbit.length == 502 and counts.max() > orbit.length
        if bla:
            assert st["steps"].sum() <= 0.5 * st["n"][esc].sum()
    if name == "seahorse-1e-12" and bla:    # level 0 only (a skip of one step), yet e is not the plain rule's 0
        assert (st["e"][esc] % 256 != 0).all()


def test_a_long_orbit_on_the_device(gpu):
    """The seahorse view of tests/test_gpu_deep_distance_bla.py at 1e-20, mrd 30 000, 16 x 16: ~3000 skips per pixel, so both
    sides of the skip's rescale run.  Normals equal the model and none is flat."""
    seahorse = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
    mrd = 30000
    orbit = DeepOrbit(*seahorse, mrd, min_span=1e-20)
    view = DeepView(1e-20, 16, 16)
    model = RL.model(orbit, view, mrd, bla=True)
    counts, normals = _check(gpu, orbit, view, mrd, True, model, "seahorse 1e-20, mrd 30000")
    st = model[4]
    assert (counts > 1000).all() and (st["steps"] < 0.5 * st["n"]).all()
    assert (np.abs(np.hypot(normals[..., 0], normals[..., 1]) - 1.0) <= 4 * np.finfo(np.float64).eps).all()


@pytest.mark.parametrize("bla", RULES)
def test_ragged_views_and_windows(gpu, bla):
    orbit, _, mrd = _orbit("i-1e-200")
    # 61 x 45: partial 8x8 blocks on both edges; a single row.  mrd 540 leaves about a quarter of the pixels without a count
    for view in (DeepView(1e-200, 61, 45), DeepView(1e-200, 64, 1)):
        model = RL.model(orbit, view, 540, bla=bla)
        assert 0.1 < (model[1] == 0).mean() < 0.9
        _check(gpu, orbit, view, 540, bla, model, (view.width, view.height, bla))
    view = _orbit("i-1e-200")[1]
    wc, whole = _whole(gpu, "i-1e-200", bla)
    for window in ((5, 3, 21, 17), (0, 37, 64, 1)):
        c0, r0, nc, nr = window
        counts, normals, nu, rel, st = gpu.compute_deep_view_normals(orbit, view, mrd, window=window, bla=bla, want_smooth=True,
                                                                     want_distance=True)
        assert np.array_equal(counts, wc[r0:r0 + nr, c0:c0 + nc]) and _same_bits(normals, whole[r0:r0 + nr, c0:c0 + nc]), window
        assert _same_bits(rel, _distance(gpu, orbit, view, mrd, bla, window)[0])
        assert _same_bits(nu, gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, want_smooth=True, bla=bla)[2])
        assert st.pixel_iterations == int(np.where(counts > 0, counts, mrd - 1).astype(np.int64).sum())


@pytest.mark.parametrize("centre, span_r, span_i, mrd", [(("-2", "0"), 1e-10, None, 1000), (("-0.75", "0"), 1e-25, 4e-3, 5000)],
                         ids=["M == 1", "-0.75 span_i 4e-3"])
def test_no_skip_identity_on_the_device(gpu, centre, span_r, span_i, mrd):
    """An orbit of length 1 (no table: the plain kernel whatever the flag) and a view whose offsets never pass level 0's radius
    (the skipping kernel, plain side only): bit for bit the plain rule."""
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i or span_r))
    assert (orbit.length == 1) == (span_i is None)
    view = DeepView(span_r, 32, 32, span_i)
    a = gpu.compute_deep_view_normals(orbit, view, mrd, bla=True, want_smooth=True, want_distance=True)
    b = gpu.compute_deep_view_normals(orbit, view, mrd, bla=False, want_smooth=True, want_distance=True)
    assert np.array_equal(a[0], b[0]) and (a[0] > 0).any()
    for x, y in zip(a[1:4], b[1:4]):
        assert _same_bits(x, y)
    want, mn, _, _, _ = RL.model(orbit, view, mrd)
    assert np.array_equal(a[0], mn) and _same_bits(a[1], want)


def test_launch_on_a_torch_stream_with_guards(gpu):
    """Into sentinel-filled buffers with guard rows in front of and behind the window, for each combination of NULL optional
    outputs: every element of the window is written, flat normals included, and nothing outside it."""
    import torch
    orbit, view, _ = _orbit("seahorse-1e-12")
    mrd = 480                   # about a tenth of the pixels never escape: their flat normals, zero nu and zero rel are written too
    guard = 3 * 64
    stream = torch.cuda.Stream(device="cuda:0")
    for bla in RULES:
        model = RL.model(orbit, view, mrd, bla=bla)
        assert 0.02 < (model[1] == 0).mean() < 0.5
        wc, whole = _check(gpu, orbit, view, mrd, bla, model, ("launch", bla))
        for window in (None, (5, 3, 21, 17)):
            c0, r0, nc, nr = window or (0, 0, view.width, view.height)
            want, want_c = whole[r0:r0 + nr, c0:c0 + nc], wc[r0:r0 + nr, c0:c0 + nc]
            px = want_c.size
            _, _, nu, rel, _ = gpu.compute_deep_view_normals(orbit, view, mrd, window=window, bla=bla, want_smooth=True, want_distance=True)
            forms = [(wc_, ws, wr) for wc_ in (True, False) for ws in (True, False) for wr in (True, False)]
            bufs = [(torch.full((2 * (px + 2 * guard),), -77.0, dtype=torch.float64, device="cuda:0"),
                     torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0"),
                     torch.full((px + 2 * guard,), -78.0, dtype=torch.float64, device="cuda:0"),
                     torch.full((px + 2 * guard,), -79.0, dtype=torch.float64, device="cuda:0")) for _ in forms]
            torch.cuda.synchronize()
            for (dn, dc, ds, dr), (with_c, with_s, with_r) in zip(bufs, forms):
                gpu.launch_deep_view_normals(orbit, view, mrd, d_normals=dn[2 * guard:].data_ptr(),
                                             d_counts=dc[guard:].data_ptr() if with_c else 0,
                                             d_smooth=ds[guard:].data_ptr() if with_s else 0,
                                             d_rel=dr[guard:].data_ptr() if with_r else 0, stream=stream.cuda_stream, window=window, bla=bla)
            stream.synchronize()
            for (dn, dc, ds, dr), form in zip(bufs, forms):
                hn, hc, hs, hr = (t.cpu().numpy() for t in (dn, dc, ds, dr))
                assert _same_bits(hn[2 * guard:2 * (guard + px)].reshape(want.shape), want), (bla, window, form)
                assert (hn[:2 * guard] == -77.0).all() and (hn[2 * (guard + px):] == -77.0).all(), (bla, window, form)
                for h, sentinel, given, ref in ((hc, -5, form[0], want_c), (hs, -78.0, form[1], nu), (hr, -79.0, form[2], rel)):
                    assert (h[:guard] == sentinel).all() and (h[guard + px:] == sentinel).all(), (bla, window, form)
                    if given:
                        got = h[guard:guard + px].reshape(ref.shape)
                        assert np.array_equal(got, ref) if ref.dtype == np.int32 else _same_bits(got, ref), (bla, window, form)
                    else:
                        assert (h == sentinel).all(), (bla, window, form)


@pytest.mark.parametrize("bla", RULES)
def test_shallow_mrd(gpu, bla):
    orbit = DeepOrbit("0.5", "0.5", 100, min_span=1e-3)          # outside the set: the centre escapes at its fourth step
    assert orbit.length >= 2                                      # (so there is a table)
    view = DeepView(1e-3, 16, 16)
    for mrd in (0, 1, 2, 5):
        for window in (None, (2, 3, 11, 9)):
            counts, normals, nu, rel, st = gpu.compute_deep_view_normals(orbit, view, mrd, window=window, bla=bla, want_smooth=True,
                                                                         want_distance=True)
            want, mn, mnu, _, _ = RL.model(orbit, view, mrd, window, bla=bla)
            assert np.array_equal(counts, mn) and _same_bits(normals, want)
            if mrd < 2:
                assert not counts.any() and not normals.any() and not nu.any() and not rel.any()
                assert st.pixel_iterations == 0 and st.never_pixels == counts.size
    assert mn.max() > 0 and (want[mn > 0] != 0.0).any(axis=1).all()          # (mrd 5: pixels have escaped, with unit normals)


def _render_palette():
    rng = np.random.RandomState(11)
    return Palette(rng.randint(0, 256, (53, 4)).astype(np.uint8), inside=(9, 8, 7, 200), scale=3.7, offset=0.25)


@pytest.mark.parametrize("bla", RULES)
@pytest.mark.parametrize("s", [1, 2, 3])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s, bla):
    orbit, mrd = _orbit("seahorse-1e-12")[0], 480          # (about a tenth of the samples never escape)
    w, h = 40, 28
    view = DeepView(1e-12, w, h)
    fine = DeepView(1e-12, w * s, h * s, view.span_i)
    pal = _render_palette()
    counts, normals, nu, st_s = gpu.compute_deep_view_normals(orbit, fine, mrd, bla=bla, want_smooth=True)
    assert (counts == 0).any() and len(np.unique(counts)) > 10
    light, height = (math.cos(0.6), math.sin(0.6)), 1.25
    want = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=normals, light=light, height=height)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    for rows in (0, 3):
        img, st = gpu.render_deep_view_relief(orbit, view, mrd, palette=pal, light=light, height=height, supersample=s, bla=bla,
                                              max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (7, 5, 19, 13)
    img, _ = gpu.render_deep_view_relief(orbit, view, mrd, palette=pal, light=light, height=height, supersample=s, bla=bla, window=window)
    assert np.array_equal(img, want[5:18, 7:26])
    # the launch form on a caller's stream, guard words behind the image
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_deep_view_relief(orbit, view, mrd, palette=pal, d_rgba=d.data_ptr(), light=light, height=height, supersample=s,
                                       bla=bla, stream=stream.cuda_stream, max_band_rows=5)
    stream.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


@pytest.mark.parametrize("bla", RULES)
def test_the_neutral_shade(gpu, bla):
    """height 2^10 without a light: every escaped sample takes the neutral q = 255 -- the smooth image scaled by 255 / 256 --
    and the inside colour none."""
    orbit, mrd = _orbit("seahorse-1e-12")[0], 480
    view = DeepView(1e-12, 40, 28)
    pal = _render_palette()
    flat, _ = gpu.render_deep_view_relief(orbit, view, mrd, palette=pal, light=(0.0, 0.0), height=2.0 ** 10, bla=bla)
    smooth, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source="smooth", bla=bla)
    counts, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False, bla=bla)
    assert RM.neutral(2.0 ** 10) == 255
    want = smooth.astype(np.int64)
    want[..., :3] = (want[..., :3] * 255 + 128) >> 8
    want[counts == 0] = pal.inside
    assert np.array_equal(flat, want) and (counts == 0).any() and (counts > 0).any()
    lit, _ = gpu.render_deep_view_relief(orbit, view, mrd, palette=pal, bla=bla)                 # 45 degrees, height 1.5
    assert (lit != flat).any(axis=2).sum() > 200


def test_refusals_write_nothing(gpu):
    """Argument checks that return before any launch: status, message, nothing written, and the ctx works afterwards."""
    import torch
    lib = gpu._lib
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    view = DeepView(1e-20, 16, 16)
    cv = gpu._cdeep(view, None)
    guard = 64
    dn = torch.full((2 * (256 + 2 * guard),), -77.0, dtype=torch.float64, device="cuda:0")
    dd = torch.full((256 + 2 * guard,), -78.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((256 + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    di = torch.full((256 + 2 * guard,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pn, pd, pc, pi = dn[2 * guard:].data_ptr(), dd[guard:].data_ptr(), dc[guard:].data_ptr(), di[guard:].data_ptr()
    launch, compute = lib.mbk_deep_view_launch_normal, lib.mbk_deep_view_compute_normal
    rl, rc = lib.mbk_deep_view_relief_render_launch, lib.mbk_deep_view_relief_render_compute
    hn, h, hc, himg = np.full(512, -1.0), np.full(256, -2.0), np.full(256, -9, np.int32), np.full((16, 16, 4), 3, np.uint8)
    pal = _render_palette()
    spec = pal.relief_spec(1)

    def refused(st, message=None):
        assert st == L.MBK_ERR_INVALID
        if message is not None:
            assert _error_text(lib, gpu._h) == message

    # a NULL normal, spec, palette or output pointer
    refused(launch(gpu._h, orbit._h, C.byref(cv), 100, 0, pc, None, pd, pd, None), "NULL normal pointer")
    refused(compute(gpu._h, orbit._h, C.byref(cv), 100, 0, hc.ctypes.data, None, h.ctypes.data, h.ctypes.data, None), "NULL normal pointer")
    with pytest.raises(MbkError):
        gpu.launch_deep_view_normals(orbit, view, 100, d_normals=0, d_counts=pc)
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, None, pi, None), "render spec is NULL")
    refused(rc(gpu._h, orbit._h, C.byref(cv), 100, 0, None, himg.ctypes.data, None), "render spec is NULL")
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), None, None), "output pointer is NULL")
    refused(rc(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), None, None), "output pointer is NULL")
    no_palette = pal.relief_spec(1)
    no_palette.palette = None
    # a light or a height outside the ranges of the plain relief renders, and what a smooth render refuses of a spec
    bad_specs = [no_palette, pal.relief_spec(5), pal.relief_spec(1, light=(1.5, 0.0)), pal.relief_spec(1, light=(0.0, math.nan)),
                 pal.relief_spec(1, light=(math.inf, 0.0)), pal.relief_spec(1, height=-0.5), pal.relief_spec(1, height=2.0 ** 10 + 1),
                 pal.relief_spec(1, height=math.nan), pal.relief_spec(1, height=math.inf), Palette(pal.entries[:1]).relief_spec(1),
                 Palette(pal.entries, scale=0.0).relief_spec(1), Palette(pal.entries, offset=math.nan).relief_spec(1)]
    for bad in bad_specs:
        for flags in (0, L.MBK_DEEP_BLA):
            refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(bad), pi, None))
            refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(bad), himg.ctypes.data, None))
    # any flag bit other than MBK_DEEP_BLA
    only = "deep normals take MBK_DEEP_BLA only (no kernel selection, no fp32)"
    render_only = "deep renders take MBK_DEEP_BLA only (no kernel selection, no fp32)"
    for flags in (L.MBK_WANT_COUNTS, L.MBK_WANT_BYTES, L.MBK_KERNEL_GROUP, L.MBK_DEEP_XBLA, L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM,
                  L.MBK_DEEP_BLA | L.MBK_WANT_COUNTS, L.MBK_DEEP_BLA | L.MBK_DEEP_XBLA, 0x80000000):
        refused(launch(gpu._h, orbit._h, C.byref(cv), 100, flags, pc, pn, pd, pd, None), only)
        refused(compute(gpu._h, orbit._h, C.byref(cv), 100, flags, hc.ctypes.data, hn.ctypes.data, h.ctypes.data, h.ctypes.data, None), only)
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), pi, None), render_only)
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), himg.ctypes.data, None), render_only)
    # whatever mbk_deep_view_launch_distance refuses for the view, the orbit and mrd; ranges below 2^-960 are a wide view's
    views = [(dict(mrd=501), "mrd exceeds the mrd the reference orbit was computed for"),
             (dict(ncols=0), "empty window"), (dict(col0=10, ncols=7), "window exceeds the view"), (dict(width=0), "empty view"),
             (dict(range_r=2.0 ** -961), "deep view ranges must be finite and lie in [2^-960, 4]"),
             (dict(range_i=4.5), "deep view ranges must be finite and lie in [2^-960, 4]"),
             (dict(range_r=math.nan), "deep view ranges must be finite and lie in [2^-960, 4]")]
    ok = dict(range_r=1e-20, range_i=1e-20, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16)
    for change, text in views:
        f = dict(ok, **change)
        bad = L.mbk_deep_view(*[f[k] for k in ("range_r", "range_i", "width", "height", "col0", "row0", "ncols", "nrows")])
        for flags in (0, L.MBK_DEEP_BLA):
            refused(launch(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), flags, pc, pn, pd, pd, None), text)
            refused(compute(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), flags, hc.ctypes.data, hn.ctypes.data, None, None, None), text)
            if "width" not in change:       # (a render of an empty view is refused for its geometry first)
                refused(rl(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), flags, C.byref(spec), pi, None), text)
                refused(rc(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), flags, C.byref(spec), himg.ctypes.data, None), text)
    refused(launch(gpu._h, None, C.byref(cv), 100, 0, pc, pn, pd, pd, None), "orbit is NULL")
    refused(compute(gpu._h, orbit._h, None, 100, 0, hc.ctypes.data, hn.ctypes.data, None, None, None), "view is NULL")
    refused(launch(None, orbit._h, C.byref(cv), 100, 0, pc, pn, pd, pd, None))
    refused(rl(gpu._h, None, C.byref(cv), 100, 0, C.byref(spec), pi, None), "orbit is NULL")
    refused(rc(gpu._h, orbit._h, None, 100, 0, C.byref(spec), himg.ctypes.data, None), "view is NULL")
    refused(launch(gpu._h, orbit._h, C.byref(cv), 100, 0, pc, pn + 4, pd, pd, None), "d_normal must be 8-byte aligned")
    with pytest.raises(MbkError):
        gpu.compute_deep_view_normals(orbit, view, 501)
    with pytest.raises(MbkError):
        gpu.render_deep_view_relief(orbit, view, 100, palette=pal, height=-1.0)
    with pytest.raises(MbkError):
        gpu.render_deep_view_relief(orbit, view, 100, palette=pal, window=(10, 0, 7, 16))

    # a WideDeepView: MbkError with a message that names the limit, before the C call; xbla is no parameter
    wide = WideDeepView(1.0, -1100, 16, 16)
    for call in (lambda: gpu.compute_deep_view_normals(orbit, wide, 100),
                 lambda: gpu.launch_deep_view_normals(orbit, wide, 100, d_normals=pn, d_counts=pc),
                 lambda: gpu.render_deep_view_relief(orbit, wide, 100, palette=pal),
                 lambda: gpu.launch_render_deep_view_relief(orbit, wide, 100, palette=pal, d_rgba=pi)):
        with pytest.raises(MbkError, match="DeepView only.*2\\^-960"):
            call()
    with pytest.raises(TypeError):
        gpu.compute_deep_view_normals(orbit, view, 100, xbla=True)

    torch.cuda.synchronize()
    assert (dn.cpu().numpy() == -77.0).all() and (dd.cpu().numpy() == -78.0).all() and (dc.cpu().numpy() == -5).all()
    assert (di.cpu().numpy() == -3).all() and (hn == -1.0).all() and (h == -2.0).all() and (hc == -9).all() and (himg == 3).all()
    # the ctx works afterwards
    for bla in RULES:
        counts, normals, _ = gpu.compute_deep_view_normals(orbit, view, 100, bla=bla)
        want, mn, _, _, _ = RL.model(orbit, view, 100, bla=bla)
        assert np.array_equal(counts, mn) and _same_bits(normals, want)
        img, _ = gpu.render_deep_view_relief(orbit, view, 100, palette=pal, bla=bla)
        assert img.shape == (16, 16, 4)
