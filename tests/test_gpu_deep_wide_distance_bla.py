"""Distance estimates for extended-range deep views with bilinear approximation on the GPU (include/mbk.h, the section of that
name), held to the numpy model of the contract (tests/deep_wide_distance_bla_model.py).

The counts are compared with the model's and with compute_deep_view(xbla=True)'s bit for bit.  The states behind rel (zp, D, e,
mag, dmagD) are exact in the model, so the device's rel must be the model's value wherever ocml's ln and numpy's agree, and
elsewhere the value a neighbouring ln gives (assert_states_agree).  Views are 24 x 20 unless said, 16 x 12 at exp2 -3000: the
smallest that still hold partial 8x8 blocks, a rebase, m == M and a climb over several levels.

Measured on gfx950 (ocml, ROCm 7): every sample of every case, window, thin view and of the M == 1 orbit equals the numpy model
bit for bit (ocml's ln met numpy's on all of them); 0.043 / 0.042 / 0.016 of the reference's iterations are executed on
"i-1100" / "mis-1100" / "i-3000", all of them on "1e-400".
"""
import ctypes as C

import numpy as np
import pytest

import deep_wide_distance_bla_model as XD
from distributedmandelbrot_amd import DeepOrbit, MandelbrotDevice, MbkError, Palette, WideDeepView
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
        rel, c, _ = gpu.compute_wide_view_distance_xbla(orbit, view, mrd)
        rel.setflags(write=False)
        c.setflags(write=False)
        _cache["whole", name] = (rel, c)
    return _cache["whole", name]


def _model(orbit, view, mrd, window=None, key=None):
    """The model of (orbit, view, mrd, window); with a key it is computed once and shared."""
    if key is None:
        return XD.model(orbit, view, mrd, window)
    if ("model", key) not in _cache:
        out = XD.model(orbit, view, mrd, window)
        for a in (out[0], out[1]) + tuple(out[2].values()):
            a.setflags(write=False)
        _cache["model", key] = out
    return _cache["model", key]


def _check(gpu, orbit, view, mrd, window, what, key=None):
    rel, c, stats = gpu.compute_wide_view_distance_xbla(orbit, view, mrd, window=window)
    ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, xbla=True)
    mrel, mn, st = _model(orbit, view, mrd, window, key)
    assert rel.shape == c.shape == mn.shape and rel.dtype == np.float64 and c.dtype == np.int32
    assert np.array_equal(c, ref), (what, int((c != ref).sum()))
    assert np.array_equal(c, mn), (what, int((c != mn).sum()))
    assert not np.isnan(rel).any() and (rel[c == 0] == 0.0).all() and (rel >= 0.0).all(), what
    share = XD.assert_states_agree(rel, st, view.range_r, view.exp2, what)
    refs = int(np.where(c > 0, c, max(mrd - 1, 0)).astype(np.int64).sum())
    print(f"{what}: {100 * share:.2f} % of the samples equal the numpy model bit for bit, e {int(st['e'].min())}..{int(st['e'].max())}, "
          f"{len(np.unique(c))} distinct counts, {int((c > 0).sum())} of {c.size} escaped, steps executed / reference iterations "
          f"{st['steps'].sum() / max(refs, 1):.4f}")
    assert stats.pixel_iterations == refs, what            # the reference's iterations: not the steps executed, not the run-on
    assert stats.never_pixels == int((c == 0).sum()), what
    return rel, c, st


@pytest.mark.parametrize("name", list(CASES))
def test_every_sample_against_the_model(gpu, name):
    orbit, view, mrd = _orbit(name)
    rel, c, st = _check(gpu, orbit, view, mrd, None, name, key=name)
    assert (c > 0).mean() >= 0.8 and np.isfinite(rel).all() and len(np.unique(c)) >= 5
    wrel, wc = _whole(gpu, name)
    assert np.array_equal(rel, wrel) and np.array_equal(c, wc)
    if name == "1e-400":
        # no level is ever taken: the full-step launch's bits (the same ln on the same states)
        assert not st["first_skip"].any()
        frel, fc, _ = gpu.compute_wide_view_distance(orbit, view, mrd)
        assert np.array_equal(c, fc) and np.array_equal(rel.view(np.uint64), frel.view(np.uint64))
    else:
        assert (st["e"][st["n"] > 0] > -view.exp2 - 64).all()        # |d| ~ 1 / (distance to the set): far above binary64
        assert (st["first_skip"] > 0).mean() > 0.9 and st["steps"].sum() < 0.5 * np.where(c > 0, c, mrd - 1).sum()


def test_windows_equal_the_whole_view(gpu):
    orbit, view, mrd = _orbit("i-1100")
    whole, wc = _whole(gpu, "i-1100")
    for window in (RAGGED, (23, 19, 1, 1), (0, 8, 24, 8), (5, 0, 3, 20)):
        c0, r0, nc, nr = window
        rel, c, _ = gpu.compute_wide_view_distance_xbla(orbit, view, mrd, window=window)
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
        rel, c, st = gpu.compute_wide_view_distance_xbla(orbit, view, mrd)
        ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False, xbla=True)
        assert np.array_equal(c, ref)
        assert not rel.any() and not c.any() and st.never_pixels == c.size        # (no pixel of this view escapes at step 1)
        if mrd < 2:
            assert st.pixel_iterations == 0
        for window in (RAGGED, (23, 19, 1, 1)):
            wrel, wc, _ = gpu.compute_wide_view_distance_xbla(orbit, view, mrd, window=window)
            assert not wrel.any() and not wc.any() and wrel.shape == (window[3], window[2])
    # a view wide enough that pixels escape at step 1: mrd 2 against the model
    far = DeepOrbit("0", "1", 10, precision_bits=128)
    rel, c, _ = _check(gpu, far, WideDeepView(4.0, 0, 24, 20), 2, None, "mrd 2")
    assert (c == 1).any() and (c == 0).any()


def test_an_orbit_of_length_one_equals_the_call_without_xbla(gpu):
    mrd = 400
    orbit = DeepOrbit("-2", "0", mrd, min_span_exp2=-1100)
    assert orbit.length == 1
    for view, window in ((WideDeepView(1.0, -1100, 24, 20), None), (WideDeepView(1.0, -1100, 29, 23), RAGGED)):
        rel, c, _ = _check(gpu, orbit, view, mrd, window, "M == 1")
        frel, fc, _ = gpu.compute_wide_view_distance(orbit, view, mrd, window=window)
        assert (c > 0).any() and np.array_equal(c, fc) and np.array_equal(rel.view(np.uint64), frel.view(np.uint64))


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
            gpu.launch_wide_view_distance_xbla(orbit, view, mrd, d_rel=dd[guard:].data_ptr(),
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


@pytest.mark.parametrize("s", [1, 2])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s):
    """The sample view at s x is a full view of its own, with a table of its own."""
    orbit, view, mrd = _orbit("i-1100")
    w, h = view.width, view.height
    finer = WideDeepView(view.range_r, view.exp2, w * s, h * s, view.range_i)
    pal = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255)).for_deep_distance(view, 12.0)
    rel, counts, st_s = gpu.compute_wide_view_distance_xbla(orbit, finer, mrd)
    want = resolve_host(pal, "distance_rel", s, w, h, counts=counts, smooth=rel)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 50
    for rows in (0, 1, 7):
        img, st = gpu.render_wide_view_distance_xbla(orbit, view, mrd, palette=pal, supersample=s, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    c0, r0, nc, nr = RAGGED
    img, _ = gpu.render_wide_view_distance_xbla(orbit, view, mrd, palette=pal, supersample=s, window=RAGGED, max_band_rows=3)
    assert np.array_equal(img, want[r0:r0 + nr, c0:c0 + nc])
    import torch
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    gpu.launch_render_wide_view_distance_xbla(orbit, view, mrd, palette=pal, d_rgba=d.data_ptr(), supersample=s, max_band_rows=7)
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
    launch, compute = lib.mbk_deep_xview_launch_distance_xbla, lib.mbk_deep_xview_compute_distance_xbla
    h, hc, himg = np.full(256, -1.0), np.full(256, -9, np.int32), np.full((16, 16, 4), 3, np.uint8)

    def refused(st, message):
        assert (st, _error_text(lib, gpu._h)) == (L.MBK_ERR_INVALID, message)

    refused(launch(gpu._h, orbit._h, C.byref(cv), 100, 0, pc, None, None), "NULL value pointer")
    refused(compute(gpu._h, orbit._h, C.byref(cv), 100, 0, hc.ctypes.data, None, None), "NULL value pointer")
    no_flags = "extended-range deep distance estimates take no flags (no kernel selection, no fp32)"
    flag_text = [(L.MBK_DEEP_XBLA, "the _distance_xbla calls take no flags: the name selects the rule (MBK_DEEP_XBLA is a flag of the count calls)"),
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
        gpu.launch_wide_view_distance_xbla(orbit, view, 100, d_rel=0, d_counts=pc)
    with pytest.raises(MbkError):
        gpu.compute_wide_view_distance_xbla(orbit, view, 501)

    # the renders: a source other than MBK_RENDER_DISTANCE_REL, any flag, and what the sample launch refuses
    pal = Palette.deep_distance(view, 8.0)
    rl, rc = lib.mbk_deep_xview_distance_xbla_render_launch, lib.mbk_deep_xview_distance_xbla_render_compute
    only = "extended-range deep distance renders with bilinear approximation take MBK_RENDER_DISTANCE_REL only"
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
            gpu.render_wide_view_distance_xbla(orbit, view, 100, palette=bad)

    # the refusals of the existing names stand, with their messages
    old = "MBK_DEEP_XBLA is not implemented for extended-range deep distance estimates"
    refused(lib.mbk_deep_xview_launch_distance(gpu._h, orbit._h, C.byref(cv), 100, L.MBK_DEEP_XBLA, pc, pd, None), old)
    refused(lib.mbk_deep_xview_compute_distance(gpu._h, orbit._h, C.byref(cv), 100, L.MBK_DEEP_XBLA, hc.ctypes.data, h.ctypes.data, None), old)
    refused(lib.mbk_deep_xview_distance_render_launch(gpu._h, orbit._h, C.byref(cv), 100, L.MBK_DEEP_XBLA, C.byref(spec), pi, None), old)
    with pytest.raises(ValueError, match="distance estimates are not implemented for a WideDeepView"):
        gpu.compute_deep_view_distance(orbit, view, 100)
    with pytest.raises(ValueError, match="distance estimates are not implemented for a WideDeepView"):
        gpu.render_deep_view(orbit, view, 100, palette=pal, source="distance_rel")
    refused(lib.mbk_deep_xview_render_launch(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), pi, None),
            "distance estimates are not implemented for extended-range deep views")

    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all() and (di.cpu().numpy() == -3).all()
    assert (h == -1.0).all() and (hc == -9).all() and (himg == 3).all()
    # the ctx works afterwards
    rel, c, _ = gpu.compute_wide_view_distance_xbla(orbit, view, 100)
    mrel, mn, st = XD.model(orbit, view, 100)
    assert np.array_equal(c, mn)
    XD.assert_states_agree(rel, st, view.range_r, view.exp2, "after the refusals")
    img, _ = gpu.render_wide_view_distance_xbla(orbit, view, 100, palette=pal)
    assert img.shape == (16, 16, 4)


def test_the_table_is_shared_with_the_count_launches(gpu):
    """A count launch with xbla=True and a distance launch in turn on one orbit: first on one set of spans (one table, built
    once by whichever comes first), then on two (the table is rebuilt at every change of dcmax).  Every result equals that of
    a fresh context."""
    orbit, view, mrd = _orbit("i-1100")
    other = WideDeepView(1.0, -1090, 24, 20)
    with MandelbrotDevice(0) as fresh:
        want = {}
        for k, v in enumerate((view, other)):
            rel, c, _ = fresh.compute_wide_view_distance_xbla(orbit, v, mrd)
            want[k] = (rel, c)
    with MandelbrotDevice(0) as fresh:
        for k, v in enumerate((view, other)):
            ref = fresh.compute_deep_view(orbit, v, mrd, want_bytes=False, xbla=True)[0]
            assert np.array_equal(ref, want[k][1]), k
    assert not np.array_equal(want[0][1], want[1][1])
    mrel, mn, st = _model(orbit, view, mrd, None, "i-1100")
    assert np.array_equal(want[0][1], mn)
    XD.assert_states_agree(want[0][0], st, view.range_r, view.exp2, "fresh context")
    views = (view, other)
    for k in (0, 0, 1, 0, 1, 1):
        ref = gpu.compute_deep_view(orbit, views[k], mrd, want_bytes=False, xbla=True)[0]
        rel, c, _ = gpu.compute_wide_view_distance_xbla(orbit, views[k], mrd)
        assert np.array_equal(ref, want[k][1]) and np.array_equal(c, want[k][1]), k
        assert np.array_equal(rel.view(np.uint64), want[k][0].view(np.uint64)), k
    for k in (1, 0):                                   # the distance launch first: it builds the table the count launch reads
        rel, c, _ = gpu.compute_wide_view_distance_xbla(orbit, views[k], mrd)
        ref = gpu.compute_deep_view(orbit, views[k], mrd, want_bytes=False, xbla=True)[0]
        assert np.array_equal(ref, want[k][1]) and np.array_equal(c, want[k][1]), k
        assert np.array_equal(rel.view(np.uint64), want[k][0].view(np.uint64)), k
