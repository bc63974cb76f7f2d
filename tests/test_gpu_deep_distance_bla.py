"""Distance estimates for deep views with bilinear approximation on the GPU (include/mbk.h, the section of that name), held to
the numpy model of the contract (tests/deep_distance_bla_model.py).

The counts are compared with the model's and with compute_deep_view(bla=True)'s bit for bit.  The states behind rel (zp, D, e,
mag, dmagD) are exact in the model, so the device's rel must be the model's value wherever ocml's ln and numpy's agree, and
elsewhere the value a neighbouring ln gives (deep_distance_model.assert_states_agree).  Views are 64 x 64 or smaller, mrd at
most 3000 (5000 for the one view that takes no skip, 30 000 for one 16 x 16 view whose pixels take ~3000 skips each).
"""
import ctypes as C

import numpy as np
import pytest

import deep_distance_bla_model as DB
import deep_distance_model as DD
import distance_model as M
import render_model as R
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, WideDeepView
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _error_text
from test_deep_distance import CASES

pytestmark = pytest.mark.gpu

WHOLE = ("i-1e-200", "M51-1e-35", "seahorse-1e-12")
_cache = {}


def _orbit(name):
    if name not in _cache:
        centre, span, mrd = CASES[name]
        _cache[name] = (DeepOrbit(*centre, mrd, min_span=span), DeepView(span, 64, 64), mrd)
    return _cache[name]


def _check(gpu, orbit, view, mrd, window, what):
    rel, c, stats = gpu.compute_deep_view_distance_bla(orbit, view, mrd, window=window)
    ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, bla=True)
    mrel, mn, st = DB.model(orbit, view, mrd, window)
    assert rel.shape == c.shape == mn.shape and rel.dtype == np.float64 and c.dtype == np.int32
    assert np.array_equal(c, ref), (what, int((c != ref).sum()))
    assert np.array_equal(c, mn), (what, int((c != mn).sum()))
    assert not np.isnan(rel).any() and (rel[c == 0] == 0.0).all() and (rel >= 0.0).all(), what
    share = DD.assert_states_agree(rel, st, view.span_r, what)
    iters = np.where(c > 0, c, max(mrd - 1, 0)).astype(np.int64).sum()
    print(f"{what}: {100 * share:.2f} % of the samples equal the numpy model bit for bit, e {int(st['e'].min())}..{int(st['e'].max())}, "
          f"{len(np.unique(c))} distinct counts, steps executed / iterations {st['steps'].sum() / max(iters, 1):.3f}")
    # the statistics count the reference's iterations, not the steps executed and not the run-on
    assert stats.pixel_iterations == int(iters), what
    assert stats.never_pixels == int((c == 0).sum()), what
    return rel, c, st


def _whole(gpu, name):
    """The device's (rel, counts) of the case's whole view and the model's states: computed once, shared, left unchanged."""
    if ("whole", name) not in _cache:
        orbit, view, mrd = _orbit(name)
        rel, c, st = _check(gpu, orbit, view, mrd, None, name)
        rel.setflags(write=False)
        c.setflags(write=False)
        _cache["whole", name] = (rel, c, st)
    return _cache["whole", name]


@pytest.mark.parametrize("name", WHOLE)
def test_whole_views_every_sample(gpu, name):
    orbit, view, mrd = _orbit(name)
    rel, c, st = _whole(gpu, name)
    esc = st["n"] > 0
    assert esc.mean() >= 0.9 and np.isfinite(rel).all() and len(np.unique(c)) >= 8
    if name == "i-1e-200":          # long skips, e past 512
        assert (st["e"][esc] >= 512).all() and st["steps"].sum() <= 0.2 * st["n"][esc].sum()
    if name == "M51-1e-35":         # the orbit wraps: rebases at m == M, lanes at different m
        assert orbit.length == 502 and c.max() > orbit.length and st["steps"].sum() <= 0.5 * st["n"][esc].sum()
    if name == "seahorse-1e-12":    # level 0 only (a skip of one step), yet e is not the plain rule's 0: the skips move it by the
        assert (st["e"][esc] % 256 != 0).all()          # exponents of A


def test_a_long_orbit_on_the_device(gpu):
    """Beyond the cases of the list above: the seahorse view of scripts/deep_rate.py at 1e-20, mrd 30 000, 16 x 16.  ~3000 skips
    per pixel, so the upward side of the skip's rescale runs on the device (without it D decays to 1e-207 and rel is inf)."""
    seahorse = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
    mrd = 30000
    orbit = DeepOrbit(*seahorse, mrd, min_span=1e-20)
    rel, c, st = _check(gpu, orbit, DeepView(1e-20, 16, 16), mrd, None, "seahorse 1e-20, mrd 30000")
    top = np.maximum(np.abs(st["Dr"]), np.abs(st["Di"]))
    assert (c > 1000).all() and (st["steps"] < 0.5 * st["n"]).all()
    assert (top >= 2.0 ** -256).all() and np.isfinite(rel).all() and (rel > 0).all() and (rel < 1).all()


def test_windows_equal_the_whole_view(gpu):
    orbit, view, mrd = _orbit("i-1e-200")
    whole, wc, _ = _whole(gpu, "i-1e-200")
    # 61 x 43 at (2, 3): partial 8x8 blocks on both edges; and one row
    for window in ((2, 3, 61, 43), (0, 37, 64, 1)):
        c0, r0, nc, nr = window
        rel, c, _ = gpu.compute_deep_view_distance_bla(orbit, view, mrd, window=window)
        assert np.array_equal(c, wc[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(rel.view(np.uint64), whole[r0:r0 + nr, c0:c0 + nc].view(np.uint64)), window


@pytest.mark.parametrize("centre, span_r, span_i, mrd", [(("-2", "0"), 1e-10, None, 1000), (("-0.75", "0"), 1e-25, 4e-3, 5000)],
                         ids=["M == 1", "-0.75 span_i 4e-3"])
def test_no_skip_identity_on_the_device(gpu, centre, span_r, span_i, mrd):
    """An orbit of length 1 (no table: the launch is deep_distance_kernel's) and a view whose offsets never pass level 0's radius
    (the new kernel, plain side only): bit for bit what compute_deep_view_distance stores."""
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i or span_r))
    assert (orbit.length == 1) == (span_i is None)
    view = DeepView(span_r, 64, 64, span_i)
    rel, c, st = gpu.compute_deep_view_distance_bla(orbit, view, mrd)
    prel, pc, pst = gpu.compute_deep_view_distance(orbit, view, mrd)
    assert np.array_equal(c, pc) and (c > 0).any()
    assert np.array_equal(rel.view(np.uint64), prel.view(np.uint64)), int((rel != prel).sum())
    assert (st.pixel_iterations, st.never_pixels) == (pst.pixel_iterations, pst.never_pixels)


def test_shallow_mrd(gpu):
    orbit, view, _ = _orbit("i-1e-200")
    for mrd in (0, 1):
        for window in (None, (2, 3, 61, 43)):
            rel, c, st = gpu.compute_deep_view_distance_bla(orbit, view, mrd, window=window)
            assert not rel.any() and not c.any() and st.pixel_iterations == 0 and st.never_pixels == c.size


def test_launch_on_a_torch_stream_with_guards(gpu):
    import torch
    orbit, view, mrd = _orbit("i-1e-200")
    whole, wc, _ = _whole(gpu, "i-1e-200")
    guard = 1024
    stream = torch.cuda.Stream(device="cuda:0")
    for window in (None, (2, 3, 61, 43), (63, 63, 1, 1)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        want, want_c = whole[r0:r0 + nr, c0:c0 + nc], wc[r0:r0 + nr, c0:c0 + nc]
        px = want.size
        bufs = [(torch.full((px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0"),
                 torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")) for _ in range(2)]
        torch.cuda.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            gpu.launch_deep_view_distance_bla(orbit, view, mrd, d_rel=dd[guard:].data_ptr(),
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


def test_two_spans_in_turn_each_get_their_own_table(gpu):
    """Two views of one orbit whose spans differ, alternating on one ctx, with a count launch of the same table between them:
    the table is rebuilt on every change of dcmax and shared with the count launches."""
    mrd = 3000
    orbit = DeepOrbit("0", "1", mrd, min_span=1e-30)
    views = [DeepView(1e-30, 40, 24), DeepView(1e-12, 40, 24)]
    models = [DB.model(orbit, v, mrd) for v in views]
    assert not np.array_equal(models[0][1], models[1][1])
    for k in (0, 1, 0, 1):
        rel, c, _ = gpu.compute_deep_view_distance_bla(orbit, views[k], mrd)
        assert np.array_equal(c, models[k][1]), k
        DD.assert_states_agree(rel, models[k][2], views[k].span_r, f"span {views[k].span_r:g}")
        ref, _, _, _ = gpu.compute_deep_view(orbit, views[k], mrd, want_bytes=False, bla=True)
        assert np.array_equal(ref, c), k


@pytest.mark.parametrize("s", [1, 2])
def test_render_equals_the_colour_rule_on_the_devices_own_samples(gpu, s):
    orbit, _, mrd = _orbit("i-1e-200")
    w, h = 61, 45
    view = DeepView(1e-200, w, h)
    finer = DeepView(1e-200, w * s, h * s, view.span_i)
    pal = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255)).for_deep_distance(view, 20.0)
    rel, counts, st_s = gpu.compute_deep_view_distance_bla(orbit, finer, mrd)
    assert len(np.unique(counts)) > 8
    want = R.resolve(M.colour_distance(pal.entries, pal.inside, pal.scale, pal.offset, counts, rel), s)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 50
    for rows in (0, 13):            # 13 rows: 4 bands
        img, st = gpu.render_deep_view_distance_bla(orbit, view, mrd, palette=pal, supersample=s, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (20, 10, 41, 33)
    img, _ = gpu.render_deep_view_distance_bla(orbit, view, mrd, palette=pal, supersample=s, window=window, max_band_rows=7)
    assert np.array_equal(img, want[10:43, 20:61])
    import torch
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    gpu.launch_render_deep_view_distance_bla(orbit, view, mrd, palette=pal, d_rgba=d.data_ptr(), supersample=s, max_band_rows=13)
    torch.cuda.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


def test_refusals_write_nothing(gpu):
    """Argument checks that return before any launch: status, message, nothing written, and the ctx works afterwards."""
    import torch
    lib = gpu._lib
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    view = DeepView(1e-20, 16, 16)
    cv = gpu._cdeep(view, None)
    guard = 64
    dd = torch.full((256 + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((256 + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    di = torch.full((256 + 2 * guard,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pd, pc, pi = dd[guard:].data_ptr(), dc[guard:].data_ptr(), di[guard:].data_ptr()
    launch, compute = lib.mbk_deep_view_launch_distance_bla, lib.mbk_deep_view_compute_distance_bla
    rl, rc = lib.mbk_deep_view_distance_bla_render_launch, lib.mbk_deep_view_distance_bla_render_compute
    h, hc, himg = np.full(256, -1.0), np.full(256, -9, np.int32), np.full((16, 16, 4), 3, np.uint8)
    pal = Palette.deep_distance(view, 8.0)
    spec = pal.spec("distance_rel", 1)

    def refused(st, message):
        assert (st, _error_text(lib, gpu._h)) == (L.MBK_ERR_INVALID, message)

    refused(launch(gpu._h, orbit._h, C.byref(cv), 100, 0, pc, None, None), "NULL value pointer")
    refused(compute(gpu._h, orbit._h, C.byref(cv), 100, 0, hc.ctypes.data, None, None), "NULL value pointer")
    with pytest.raises(MbkError):
        gpu.launch_deep_view_distance_bla(orbit, view, 100, d_rel=0, d_counts=pc)
    the_name = "the _distance_bla calls take no flags: the name selects the rule (MBK_DEEP_BLA is a flag of the count calls)"
    no_flags = "deep distance estimates take no flags (no kernel selection, no fp32)"
    for flags, text in ((L.MBK_DEEP_BLA, the_name), (L.MBK_WANT_COUNTS, no_flags), (L.MBK_KERNEL_GROUP, no_flags),
                        (L.MBK_DEEP_BLA | L.MBK_WANT_COUNTS, the_name), (L.MBK_DEEP_XBLA, no_flags), (L.MBK_PRECISION_F32, no_flags)):
        refused(launch(gpu._h, orbit._h, C.byref(cv), 100, flags, pc, pd, None), text)
        refused(compute(gpu._h, orbit._h, C.byref(cv), 100, flags, hc.ctypes.data, h.ctypes.data, None), text)
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), pi, None), text)
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, flags, C.byref(spec), himg.ctypes.data, None), text)
    views = [(dict(mrd=501), "mrd exceeds the mrd the reference orbit was computed for"),
             (dict(ncols=0), "empty window"), (dict(col0=10, ncols=7), "window exceeds the view"),
             (dict(range_r=2.0 ** -961), "deep view ranges must be finite and lie in [2^-960, 4]"),
             (dict(range_i=4.5), "deep view ranges must be finite and lie in [2^-960, 4]")]
    ok = dict(range_r=1e-20, range_i=1e-20, width=16, height=16, col0=0, row0=0, ncols=16, nrows=16)
    for change, text in views:
        f = dict(ok, **change)
        bad = L.mbk_deep_view(*[f[k] for k in ("range_r", "range_i", "width", "height", "col0", "row0", "ncols", "nrows")])
        refused(launch(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), 0, pc, pd, None), text)
        refused(compute(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), 0, hc.ctypes.data, h.ctypes.data, None), text)
        refused(rl(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), 0, C.byref(spec), pi, None), text)
        refused(rc(gpu._h, orbit._h, C.byref(bad), f.get("mrd", 100), 0, C.byref(spec), himg.ctypes.data, None), text)
    refused(launch(gpu._h, None, C.byref(cv), 100, 0, pc, pd, None), "orbit is NULL")
    refused(compute(gpu._h, orbit._h, None, 100, 0, hc.ctypes.data, h.ctypes.data, None), "view is NULL")
    with pytest.raises(MbkError):
        gpu.compute_deep_view_distance_bla(orbit, view, 501)
    with pytest.raises(MbkError):
        gpu.compute_deep_view_distance_bla(orbit, DeepView(2.0 ** -961, 16, 16), 100)

    # the renders: a source other than MBK_RENDER_DISTANCE_REL
    only = "deep distance renders with bilinear approximation take MBK_RENDER_DISTANCE_REL only"
    for source in ("smooth", "distance"):
        other = pal.spec(source, 1)
        refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(other), pi, None), only)
        refused(rc(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(other), himg.ctypes.data, None), only)
    other = Palette(np.zeros((256, 4), np.uint8)).spec("bytes", 1)
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(other), pi, None), only)
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, None, pi, None), "render spec is NULL")
    refused(rl(gpu._h, orbit._h, C.byref(cv), 100, 0, C.byref(spec), None, None), "output pointer is NULL")
    refused(rc(gpu._h, orbit._h, None, 100, 0, C.byref(spec), himg.ctypes.data, None), "view is NULL")

    # a WideDeepView has no such methods' kernel: refused in Python, before the C call
    wide = WideDeepView(1.0, -1100, 16, 16)
    for call in (lambda: gpu.compute_deep_view_distance_bla(orbit, wide, 100),
                 lambda: gpu.launch_deep_view_distance_bla(orbit, wide, 100, d_rel=pd, d_counts=pc),
                 lambda: gpu.render_deep_view_distance_bla(orbit, wide, 100, palette=pal),
                 lambda: gpu.launch_render_deep_view_distance_bla(orbit, wide, 100, palette=pal, d_rgba=pi)):
        with pytest.raises(ValueError, match="implemented for a DeepView only"):
            call()

    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all() and (di.cpu().numpy() == -3).all()
    assert (h == -1.0).all() and (hc == -9).all() and (himg == 3).all()
    # the ctx works afterwards
    rel, c, _ = gpu.compute_deep_view_distance_bla(orbit, view, 100)
    mrel, mn, st = DB.model(orbit, view, 100)
    assert np.array_equal(c, mn)
    DD.assert_states_agree(rel, st, view.span_r, "after the refusals")
    img, _ = gpu.render_deep_view_distance_bla(orbit, view, 100, palette=pal)
    assert img.shape == (16, 16, 4)


def test_the_old_refusals_stand(gpu):
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    view = DeepView(1e-20, 16, 16)
    cv = gpu._cdeep(view, None)
    h, hc = np.full(256, -1.0), np.full(256, -9, np.int32)
    assert gpu._lib.mbk_deep_view_compute_distance(gpu._h, orbit._h, C.byref(cv), 100, L.MBK_DEEP_BLA, hc.ctypes.data, h.ctypes.data,
                                                   None) == L.MBK_ERR_INVALID
    assert (h == -1.0).all() and (hc == -9).all()
    with pytest.raises(MbkError):
        gpu.render_deep_view(orbit, view, 100, palette=Palette.deep_distance(view, 8.0), source="distance_rel", bla=True)
