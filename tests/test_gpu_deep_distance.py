"""Distance estimates for deep views on the GPU (include/mbk.h, "Distance estimates for deep views"), held to the numpy model
of the contract (tests/deep_distance_model.py).

The counts are compared with the model's and with compute_deep_view's bit for bit.  The states behind rel (z, D, e, mag,
dmagD) are exact in the model, so the device's rel must be the model's value wherever ocml's ln and numpy's agree, and
elsewhere the value a neighbouring ln gives (deep_distance_model.assert_states_agree).

Measured on gfx950 (ocml, ROCm 7): 99.87 % .. 100 % of the samples of every small case (64 x 64, ragged windows, M == 1) equal
the numpy model bit for bit and the rest are a neighbouring ln's value; e reaches 512 at span 1e-200 and 768 at 1e-280; all
2048 seeded samples of the 4096 x 4096 view equal the model bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import deep_distance_model as DD
import deep_model as D
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import resolve_host
from test_deep_distance import CASES

pytestmark = pytest.mark.gpu

RAGGED = (7, 11, 61, 37)          # a window at an odd offset whose sides are no multiples of 8


def _check(gpu, orbit, view, mrd, window, what):
    rel, c, stats = gpu.compute_deep_view_distance(orbit, view, mrd, window=window)
    ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False)
    mrel, mn, st = DD.model(orbit, view, mrd, window)
    assert rel.shape == c.shape == mn.shape and rel.dtype == np.float64 and c.dtype == np.int32
    assert np.array_equal(c, ref), (what, int((c != ref).sum()))
    assert np.array_equal(c, mn), (what, int((c != mn).sum()))
    assert not np.isnan(rel).any() and (rel[c == 0] == 0.0).all() and (rel >= 0.0).all(), what
    share = DD.assert_states_agree(rel, st, view.span_r, what)
    print(f"{what}: {100 * share:.2f} % of the samples equal the numpy model bit for bit, e up to {int(st['e'].max())}, "
          f"{len(np.unique(c))} distinct counts")
    assert stats.pixel_iterations == int(np.where(c > 0, c, max(mrd - 1, 0)).astype(np.int64).sum()), what
    assert stats.never_pixels == int((c == 0).sum()), what
    return rel, c, st


@pytest.mark.parametrize("name", list(CASES))
def test_small_views_every_sample(gpu, name):
    centre, span, mrd = CASES[name]
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, 64, 64)
    whole, wc, st = _check(gpu, orbit, view, mrd, None, name)
    assert (wc > 0).mean() >= 0.9 and np.isfinite(whole).all()
    if name == "i-1e-200":
        assert (st["e"][st["n"] > 0] >= 512).all()
    # a ragged window and a band: bit-identical to the same pixels of the whole view
    c0, r0, nc, nr = RAGGED
    rel, c, _ = _check(gpu, orbit, DeepView(span, 80, 64), mrd, RAGGED, name + " ragged")
    for window in ((0, 24, 64, 8), (63, 63, 1, 1), (5, 0, 3, 64)):
        c0, r0, nc, nr = window
        rel, c, _ = gpu.compute_deep_view_distance(orbit, view, mrd, window=window)
        assert np.array_equal(c, wc[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(rel, whole[r0:r0 + nr, c0:c0 + nc]), window


def test_an_orbit_of_length_one(gpu):
    orbit = DeepOrbit("-2", "0", 1000, min_span=1e-10)
    assert orbit.length == 1
    rel, c, st = _check(gpu, orbit, DeepView(1e-10, 64, 64), 1000, None, "M == 1")
    assert (c > 0).any()
    _check(gpu, orbit, DeepView(1e-10, 80, 64), 1000, RAGGED, "M == 1 ragged")


def test_launch_on_a_torch_stream_with_guards(gpu):
    import torch
    centre, span, mrd = CASES["i-1e-200"]
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, 80, 64)
    guard = 1024
    stream = torch.cuda.Stream(device="cuda:0")
    whole, wc, _ = gpu.compute_deep_view_distance(orbit, view, mrd)
    for window in (None, RAGGED, (0, 8, 80, 8), (79, 63, 1, 1)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        want, want_c = whole[r0:r0 + nr, c0:c0 + nc], wc[r0:r0 + nr, c0:c0 + nc]
        px = want.size
        bufs = [(torch.full((px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0"),
                 torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")) for _ in range(2)]
        torch.cuda.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            gpu.launch_deep_view_distance(orbit, view, mrd, d_rel=dd[guard:].data_ptr(),
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


def test_one_full_size_view(gpu):
    """c = i at 1e-60, 4096 x 4096, mrd 3000: the counts of every pixel are compute_deep_view's, and a seeded sample of 2048
    pixels is held to the model."""
    n, mrd, span = 4096, 3000, 1e-60
    orbit = DeepOrbit("0", "1", mrd, min_span=span)
    view = DeepView(span, n, n)
    rel, c, stats = gpu.compute_deep_view_distance(orbit, view, mrd)
    ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
    assert np.array_equal(c, ref)
    assert not np.isnan(rel).any() and (rel >= 0.0).all() and np.array_equal(rel == 0.0, c == 0)
    assert stats.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
    pick = np.sort(np.random.RandomState(8).choice(n * n, 2048, replace=False))
    dr, di = D.axis_offsets(n, view.span_r, pick % n), D.axis_offsets(n, view.span_i, pick // n)
    zr, zi = orbit.table()
    st = DD.states(zr, zi, dr, di, mrd)
    assert np.array_equal(st["n"], c.ravel()[pick]) and len(np.unique(st["n"])) >= 8 and (st["n"] > 0).mean() >= 0.9
    share = DD.assert_states_agree(rel.ravel()[pick], st, span, "full size")
    print(f"full size: {100 * share:.2f} % of 2048 samples equal the numpy model bit for bit, e up to {int(st['e'].max())}")


@pytest.mark.parametrize("s", [1, 2, 4])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s):
    centre, span, mrd = CASES["i-1e-200"]
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    w, h = (157, 101) if s < 4 else (93, 61)
    view = DeepView(span, w, h)
    finer = DeepView(span, w * s, h * s, view.span_i)
    pal = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255)).for_deep_distance(view, 40.0)
    rel, counts, st_s = gpu.compute_deep_view_distance(orbit, finer, mrd)
    assert len(np.unique(counts)) > 8
    want = resolve_host(pal, "distance_rel", s, w, h, counts=counts, smooth=rel)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 50
    for rows in (0, 1, 13):
        img, st = gpu.render_deep_view(orbit, view, mrd, palette=pal, source="distance_rel", supersample=s, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (20, 10, 41, 33)
    img, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, source="distance_rel", supersample=s, window=window, max_band_rows=7)
    assert np.array_equal(img, want[10:43, 20:61])
    if s == 1:
        import torch
        d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
        gpu.launch_render_deep_view(orbit, view, mrd, palette=pal, d_rgba=d.data_ptr(), source="distance_rel", max_band_rows=13)
        torch.cuda.synchronize()
        hd = d.cpu().numpy()
        assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


def test_render_refusals(gpu):
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    dview = DeepView(1e-20, 32, 32)
    pal = Palette.deep_distance(dview, 8.0)
    with pytest.raises(MbkError) as e:
        gpu.render_deep_view(orbit, dview, 500, palette=pal, source="distance")
    assert "plain views only" in str(e.value)
    with pytest.raises(MbkError) as e:
        gpu.render_view(View(-2.0, -1.5, 3.0, 3.0, 32, 32), 100, palette=pal, source="distance_rel")
    assert "deep views only" in str(e.value)
    for bad in (Palette(pal.entries, scale=2.0 ** 81), Palette(pal.entries, scale=0.0), Palette(pal.entries[:1])):
        with pytest.raises(MbkError):
            gpu.render_deep_view(orbit, dview, 500, palette=bad, source="distance_rel")
    img, _ = gpu.render_deep_view(orbit, dview, 500, palette=pal, source="distance_rel")
    assert img.shape == (32, 32, 4)


def test_argument_errors_write_nothing_and_shallow_mrd(gpu):
    import torch
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    view = DeepView(1e-20, 16, 16)
    cv = gpu._cdeep(view, None)
    guard = 64
    dd = torch.full((256 + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((256 + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pd, pc = dd[guard:].data_ptr(), dc[guard:].data_ptr()
    launch, compute = gpu._lib.mbk_deep_view_launch_distance, gpu._lib.mbk_deep_view_compute_distance
    h, hc = np.full(256, -1.0), np.full(256, -9, np.int32)
    assert launch(gpu._h, orbit._h, C.byref(cv), 100, 0, pc, None, None) == L.MBK_ERR_INVALID           # NULL value pointer
    assert compute(gpu._h, orbit._h, C.byref(cv), 100, 0, hc.ctypes.data, None, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.launch_deep_view_distance(orbit, view, 100, d_rel=0, d_counts=pc)
    for flags in (L.KERNELS["asm"], L.KERNELS["scan"], L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM):
        assert launch(gpu._h, orbit._h, C.byref(cv), 100, flags, pc, pd, None) == L.MBK_ERR_INVALID, flags
        assert compute(gpu._h, orbit._h, C.byref(cv), 100, flags, hc.ctypes.data, h.ctypes.data, None) == L.MBK_ERR_INVALID, flags
    assert launch(gpu._h, None, C.byref(cv), 100, 0, pc, pd, None) == L.MBK_ERR_INVALID                  # NULL orbit
    assert launch(gpu._h, orbit._h, None, 100, 0, pc, pd, None) == L.MBK_ERR_INVALID                    # NULL view
    with pytest.raises(MbkError):
        gpu.launch_deep_view_distance(orbit, view, 501, d_rel=pd, d_counts=pc)                          # mrd above the orbit's
    with pytest.raises(MbkError):
        gpu.compute_deep_view_distance(orbit, view, 501)
    for span in (2.0 ** -961, 4.5, float("inf"), float("nan")):
        with pytest.raises(MbkError):
            gpu.launch_deep_view_distance(orbit, DeepView(span, 16, 16), 100, d_rel=pd, d_counts=pc)
        bad = gpu._cdeep(DeepView(span, 16, 16), None)
        assert compute(gpu._h, orbit._h, C.byref(bad), 100, 0, hc.ctypes.data, h.ctypes.data, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.launch_deep_view_distance(orbit, view, 100, d_rel=pd, window=(10, 0, 7, 16))
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all() and (h == -1.0).all() and (hc == -9).all()
    for mrd in (0, 1, 2):
        rel, c, st = gpu.compute_deep_view_distance(orbit, view, mrd)
        ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
        assert np.array_equal(c, ref)
        if mrd < 2:
            assert not rel.any() and not c.any() and st.pixel_iterations == 0 and st.never_pixels == 256
        else:
            mrel, mn, mst = DD.model(orbit, view, mrd)
            assert np.array_equal(c, mn)
            DD.assert_states_agree(rel, mst, view.span_r, "mrd 2")
