"""Distance estimates for extended-range deep views on the GPU (include/mbk.h, the section of that name), held to the numpy
model of the contract (tests/deep_wide_distance_model.py).

The counts are compared with the model's and with compute_deep_view's bit for bit.  The states behind rel (zp, D, e, mag,
dmagD) are exact in the model, so the device's rel must be the model's value wherever ocml's ln and numpy's agree, and
elsewhere the value a neighbouring ln gives (deep_wide_distance_model.assert_states_agree).  Views are 24 x 20 unless said.

Measured on gfx950 (ocml, ROCm 7): every sample of every case, window, thin view and of the M == 1 orbit equals the numpy model
bit for bit (ocml's ln met numpy's on all of them); e runs 1120 .. 1152 at exp2 -1100 and 3020 .. 3044 at -3000 on escaped
pixels, and down to 0 on the centre 1e-400 at span 4.
"""
import ctypes as C

import numpy as np
import pytest

import deep_wide_distance_model as WD
import deep_wide_model as W
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _cxview, _error_text
from distributedmandelbrot_amd.image import resolve_host
from test_deep_wide import MIS, TINY

pytestmark = pytest.mark.gpu

# name -> (centre, range, exp2, mrd, precision_bits (None: the default for the span), width, height)
CASES = {
    "i-1100": (("0", "1"), 1.0, -1100, 3000, None, 24, 20),
    "mis-1100": (MIS, 1.0, -1100, 4000, None, 24, 20),
    "1e-400": (TINY, 4.0, 0, 300, 1408, 24, 20),
    "i-3000": (("0", "1"), 1.0, -3000, 6000, None, 16, 12),
}
RAGGED = (3, 5, 13, 11)          # a window at an odd offset whose sides are no multiples of 8
_cache = {}


def _orbit(name):
    if name not in _cache:
        centre, rng, exp2, mrd, bits, w, h = CASES[name]
        view = WideDeepView(rng, exp2, w, h)
        orbit = DeepOrbit(*centre, mrd, precision_bits=bits) if bits else DeepOrbit(*centre, mrd, min_span_exp2=view.min_span_exp2)
        _cache[name] = (orbit, view, mrd)
    return _cache[name]


def _whole(gpu, name):
    """The device's (rel, counts) of the case's whole view: computed once, shared, left unchanged."""
    if ("whole", name) not in _cache:
        orbit, view, mrd = _orbit(name)
        rel, c, _ = gpu.compute_wide_view_distance(orbit, view, mrd)
        rel.setflags(write=False)
        c.setflags(write=False)
        _cache["whole", name] = (rel, c)
    return _cache["whole", name]


def _check(gpu, orbit, view, mrd, window, what):
    rel, c, stats = gpu.compute_wide_view_distance(orbit, view, mrd, window=window)
    ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False)
    mrel, mn, st = WD.model(orbit, view, mrd, window)
    assert rel.shape == c.shape == mn.shape and rel.dtype == np.float64 and c.dtype == np.int32
    assert np.array_equal(c, ref), (what, int((c != ref).sum()))
    assert np.array_equal(c, mn), (what, int((c != mn).sum()))
    assert not np.isnan(rel).any() and (rel[c == 0] == 0.0).all() and (rel >= 0.0).all(), what
    share = WD.assert_states_agree(rel, st, view.range_r, view.exp2, what)
    print(f"{what}: {100 * share:.2f} % of the samples equal the numpy model bit for bit, e {int(st['e'].min())}..{int(st['e'].max())}, "
          f"{len(np.unique(c))} distinct counts, {int((c > 0).sum())} of {c.size} escaped")
    assert stats.pixel_iterations == int(np.where(c > 0, c, max(mrd - 1, 0)).astype(np.int64).sum()), what
    assert stats.never_pixels == int((c == 0).sum()), what
    return rel, c, st


@pytest.mark.parametrize("name", list(CASES))
def test_every_sample_against_the_model(gpu, name):
    orbit, view, mrd = _orbit(name)
    rel, c, st = _check(gpu, orbit, view, mrd, None, name)
    assert (c > 0).mean() >= 0.8 and np.isfinite(rel).all() and len(np.unique(c)) >= 5
    if name != "1e-400":
        assert (st["e"][st["n"] > 0] > -view.exp2 - 64).all()        # |d| ~ 1 / (distance to the set): far above binary64
    wrel, wc = _whole(gpu, name)
    assert np.array_equal(rel, wrel) and np.array_equal(c, wc)


def test_a_ragged_window_equals_the_whole_view(gpu):
    orbit, view, mrd = _orbit("i-1100")
    whole, wc = _whole(gpu, "i-1100")
    for window in (RAGGED, (23, 19, 1, 1), (0, 8, 24, 8), (5, 0, 3, 20)):
        c0, r0, nc, nr = window
        rel, c, _ = gpu.compute_wide_view_distance(orbit, view, mrd, window=window)
        assert np.array_equal(c, wc[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(rel, whole[r0:r0 + nr, c0:c0 + nc]), window
    _check(gpu, orbit, WideDeepView(1.0, -1100, 29, 23), mrd, RAGGED, "ragged")


@pytest.mark.parametrize("w, h", [(1, 1), (1, 17), (17, 1)])
def test_thin_views(gpu, w, h):
    orbit, _, mrd = _orbit("i-1100")
    rel, c, _ = _check(gpu, orbit, WideDeepView(1.0, -1100, w, h, 1.0), mrd, None, f"{w} x {h}")
    assert (c > 0).sum() >= w * h - 1           # (the centre pixel is c = i itself)


def test_shallow_mrd(gpu):
    orbit, view, _ = _orbit("i-1100")
    for mrd in (0, 1, 2):
        rel, c, st = gpu.compute_wide_view_distance(orbit, view, mrd)
        ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
        assert np.array_equal(c, ref)
        assert not rel.any() and not c.any() and st.never_pixels == c.size        # (no pixel of this view escapes at step 1)
        if mrd < 2:
            assert st.pixel_iterations == 0
        for window in (RAGGED, (23, 19, 1, 1)):
            wrel, wc, _ = gpu.compute_wide_view_distance(orbit, view, mrd, window=window)
            assert not wrel.any() and not wc.any() and wrel.shape == (window[3], window[2])
    # a view wide enough that pixels escape at step 1: mrd 2 against the model
    far = DeepOrbit("0", "1", 10, precision_bits=128)
    rel, c, _ = _check(gpu, far, WideDeepView(4.0, 0, 24, 20), 2, None, "mrd 2")
    assert (c == 1).any() and (c == 0).any()


def test_an_orbit_of_length_one(gpu):
    mrd = 400
    view = WideDeepView(1.0, -1100, 24, 20)
    orbit = DeepOrbit("-2", "0", mrd, min_span_exp2=view.min_span_exp2)
    assert orbit.length == 1
    rel, c, _ = _check(gpu, orbit, view, mrd, None, "M == 1")
    assert (c > 0).any()
    _check(gpu, orbit, WideDeepView(1.0, -1100, 29, 23), mrd, RAGGED, "M == 1 ragged")


def test_launch_on_a_torch_stream_with_guards(gpu):
    import torch
    orbit, view, mrd = _orbit("i-1100")
    whole, wc = _whole(gpu, "i-1100")
    guard = 1024
    stream = torch.cuda.Stream(device="cuda:0")
    for window in (None, RAGGED, (0, 8, 24, 8), (23, 19, 1, 1)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        want, want_c = whole[r0:r0 + nr, c0:c0 + nc], wc[r0:r0 + nr, c0:c0 + nc]
        px = want.size
        bufs = [(torch.full((px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0"),
                 torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")) for _ in range(2)]
        torch.cuda.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            gpu.launch_wide_view_distance(orbit, view, mrd, d_rel=dd[guard:].data_ptr(),
                                          d_counts=dc[guard:].data_ptr() if with_counts else 0, stream=stream.cuda_stream,
                                          window=window)
        stream.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            hd, hc = dd.cpu().numpy(), dc.cpu().numpy()
            assert np.array_equal(hd[guard:guard + px].reshape(want.shape), want), (window, with_counts)
            assert (hd[:guard] == -77.0).all() and (hd[guard + px:] == -77.0).all(), (window, with_counts)
            assert (hc[:guard] == -5).all() and (hc[guard + px:] == -5).all(), (window, with_counts)
            if with_counts:
                assert np.array_equal(hc[guard:guard + px].reshape(want_c.shape), want_c), window
            else:
                assert (hc == -5).all(), window


def test_wide_equals_plain_on_the_device(gpu):
    """c = i at 1e-200, named as a wide view: the same device ln, so rel is equal bit for bit, and the counts are equal."""
    span, mrd = 1e-200, 3000
    orbit = DeepOrbit("0", "1", mrd, min_span=span)
    rr, ri, exp2 = W.as_wide(span, span)
    assert np.ldexp(rr, exp2) == span
    prel, pc, _ = gpu.compute_deep_view_distance(orbit, DeepView(span, 24, 20, span), mrd)
    wrel, wc, _ = gpu.compute_wide_view_distance(orbit, WideDeepView(rr, exp2, 24, 20, ri), mrd)
    assert np.array_equal(wc, pc) and (pc > 0).mean() > 0.9
    assert np.array_equal(wrel.view(np.uint64), prel.view(np.uint64)), int((wrel != prel).sum())


@pytest.mark.parametrize("s", [1, 2])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s):
    orbit, view, mrd = _orbit("i-1100")
    w, h = view.width, view.height
    finer = WideDeepView(view.range_r, view.exp2, w * s, h * s, view.range_i)
    pal = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255)).for_deep_distance(view, 12.0)
    rel, counts, st_s = gpu.compute_wide_view_distance(orbit, finer, mrd)
    want = resolve_host(pal, "distance_rel", s, w, h, counts=counts, smooth=rel)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 50
    for rows in (0, 1, 7):
        img, st = gpu.render_wide_view_distance(orbit, view, mrd, palette=pal, supersample=s, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    c0, r0, nc, nr = RAGGED
    img, _ = gpu.render_wide_view_distance(orbit, view, mrd, palette=pal, supersample=s, window=RAGGED, max_band_rows=3)
    assert np.array_equal(img, want[r0:r0 + nr, c0:c0 + nc])
    import torch
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    gpu.launch_render_wide_view_distance(orbit, view, mrd, palette=pal, d_rgba=d.data_ptr(), supersample=s, max_band_rows=7)
    torch.cuda.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


def test_refusals_write_nothing(gpu):
    """Argument checks that return before any launch: status, message, nothing written, and the ctx works afterwards."""
    import torch
    lib = gpu._lib
    orbit = DeepOrbit("0", "1", 500, min_span_exp2=-1100)
    view = WideDeepView(1.0, -1100, 16, 16)
    cv = _cxview(view)
    guard = 64
    dd = torch.full((256 + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((256 + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    di = torch.full((256 + 2 * guard,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pd, pc, pi = dd[guard:].data_ptr(), dc[guard:].data_ptr(), di[guard:].data_ptr()
    launch, compute = lib.mbk_deep_xview_launch_distance, lib.mbk_deep_xview_compute_distance
    h, hc, himg = np.full(256, -1.0), np.full(256, -9, np.int32), np.full((16, 16, 4), 3, np.uint8)

    def refused(st, message):
        assert (st, _error_text(lib, gpu._h)) == (L.MBK_ERR_INVALID, message)

    refused(launch(gpu._h, orbit._h, C.byref(cv), 100, 0, pc, None, None), "NULL value pointer")
    refused(compute(gpu._h, orbit._h, C.byref(cv), 100, 0, hc.ctypes.data, None, None), "NULL value pointer")
    no_flags = "extended-range deep distance estimates take no flags (no kernel selection, no fp32)"
    flag_text = [(L.MBK_DEEP_XBLA, "MBK_DEEP_XBLA is not implemented for extended-range deep distance estimates"),
                 (L.MBK_DEEP_BLA, "MBK_DEEP_BLA is not implemented for extended-range deep views"),
                 (L.KERNELS["asm"], no_flags), (L.KERNELS["scan"], no_flags), (L.MBK_PRECISION_F32, no_flags),
                 (L.MBK_LAZY_UNIFORM, no_flags), (L.MBK_WANT_COUNTS, no_flags), (L.MBK_WANT_BYTES, no_flags)]
    for flags, text in flag_text:
        refused(launch(gpu._h, orbit._h, C.byref(cv), 100, flags, pc, pd, None), text)
        refused(compute(gpu._h, orbit._h, C.byref(cv), 100, flags, hc.ctypes.data, h.ctypes.data, None), text)
    refused(launch(gpu._h, None, C.byref(cv), 100, 0, pc, pd, None), "orbit is NULL")
    refused(launch(gpu._h, orbit._h, None, 100, 0, pc, pd, None), "view is NULL")
    refused(compute(gpu._h, orbit._h, None, 100, 0, hc.ctypes.data, h.ctypes.data, None), "view is NULL")
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
        refused(launch(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), 0, pc, pd, None), text)
        refused(compute(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), 0, hc.ctypes.data, h.ctypes.data, None), text)
    with pytest.raises(MbkError):
        gpu.launch_wide_view_distance(orbit, view, 100, d_rel=0, d_counts=pc)
    with pytest.raises(MbkError):
        gpu.compute_wide_view_distance(orbit, view, 501)

    # the renders: a source other than MBK_RENDER_DISTANCE_REL, any flag, and what the sample launch refuses
    pal = Palette.deep_distance(view, 8.0)
    rl, rc = lib.mbk_deep_xview_distance_render_launch, lib.mbk_deep_xview_distance_render_compute
    only = "extended-range deep distance renders take MBK_RENDER_DISTANCE_REL only"
    for source in ("smooth", "distance"):
        spec = pal.spec(source, 1)
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), pi, None), only)
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), himg.ctypes.data, None), only)
    spec = Palette(np.zeros((256, 4), np.uint8)).spec("bytes", 1)
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), pi, None), only)
    spec = pal.spec("equalized", 1)
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), pi, None), "MBK_RENDER_EQUALIZED needs a table: use the equalized calls")
    spec = pal.spec("distance_rel", 1)
    for flags, text in flag_text:
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), pi, None), text)
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), himg.ctypes.data, None), text)
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, None, pi, None), "render spec is NULL")
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), None, None), "output pointer is NULL")
    refused(rc(gpu._h, orbit._h, None, 100, 0, C.byref(spec), himg.ctypes.data, None), "view is NULL")
    refused(rl(gpu._h, None, C.byref(cv), 100, 0, C.byref(spec), pi, None), "orbit is NULL")
    refused(rc(gpu._h, orbit._h, C.byref(cv), 501, 0, C.byref(spec), himg.ctypes.data, None),
            "mrd exceeds the mrd the reference orbit was computed for")
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(pal.spec("distance_rel", 5)), pi, None), "supersample must be 1, 2, 3, 4 or 8")
    for bad in (Palette(pal.entries, scale=2.0 ** 81), Palette(pal.entries, scale=0.0), Palette(pal.entries[:1])):
        with pytest.raises(MbkError):
            gpu.render_wide_view_distance(orbit, view, 100, palette=bad)

    # the refusals of the existing names stand
    with pytest.raises(ValueError, match="distance estimates are not implemented for a WideDeepView"):
        gpu.compute_deep_view_distance(orbit, view, 100)
    with pytest.raises(ValueError, match="distance estimates are not implemented for a WideDeepView"):
        gpu.render_deep_view(orbit, view, 100, palette=pal, source="distance_rel")
    spec = pal.spec("distance_rel", 1)
    refused(lib.mbk_deep_xview_render_launch(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), pi, None),
            "distance estimates are not implemented for extended-range deep views")

    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all() and (di.cpu().numpy() == -3).all()
    assert (h == -1.0).all() and (hc == -9).all() and (himg == 3).all()
    # the ctx works afterwards
    rel, c, _ = gpu.compute_wide_view_distance(orbit, view, 100)
    mrel, mn, st = WD.model(orbit, view, 100)
    assert np.array_equal(c, mn)
    WD.assert_states_agree(rel, st, view.range_r, view.exp2, "after the refusals")
    img, _ = gpu.render_wide_view_distance(orbit, view, 100, palette=pal)
    assert img.shape == (16, 16, 4)
