"""Deep-zoom views on the GPU (include/mbk.h, "Deep-zoom views"): the kernel is held bit for bit to the numpy restatement of
the contract (tests/deep_model.py) on the library's own orbit table, through every entry point."""
import numpy as np
import pytest

import deep_model as D
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, View

pytestmark = pytest.mark.gpu

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
# (centre, span, view, mrd, at least this many distinct counts)
CASES = [
    (SEAHORSE, 1e-8, (128, 128), 5000, 20),
    (SEAHORSE, 1e-20, (128, 96), 30000, 20),
    (("0", "1"), 1e-60, (64, 64), 5000, 20),          # c = i is on the boundary at every depth
    (("0", "1"), 1e-200, (256, 256), 5000, 20),
    (("1e-21", "1"), 1e-20, (100, 70), 5000, 20),     # the reference orbit escapes at M = 58: pixels rebase on m == M
    (("-2", "0"), 1e-60, (40, 24), 200, 1),           # M = 1: the start state is rebased, and every step after it
]


def _model(orbit, view, mrd, window=None):
    zr, zi = orbit.table()
    dr, di = D.offsets(view, window)
    c, mag = D.model_counts(zr, zi, dr, di, mrd)
    rows = window[3] if window else view.height
    return c.reshape(rows, -1), mag.reshape(rows, -1)


@pytest.mark.parametrize("centre, span, size, mrd, distinct", CASES)
def test_counts_bytes_smooth_equal_the_model(gpu, centre, span, size, mrd, distinct):
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, *size)
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, want_smooth=True)
    mc, mag = _model(orbit, view, mrd)
    assert np.array_equal(c, mc), int((c != mc).sum())
    assert len(np.unique(c)) >= distinct
    assert np.array_equal(b, gpu.quantise_counts(c, mrd))
    msm = D.smooth_from(mc, mag)
    assert (sm[mc == 0] == 0.0).all()
    assert np.allclose(sm, msm, rtol=0, atol=1e-12 * max(1, mrd)), float(np.abs(sm - msm).max())
    assert st.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
    assert st.never_pixels == int((c == 0).sum())
    if centre == ("1e-21", "1"):
        assert orbit.escaped and orbit.length == 58 and c.max() > orbit.length
    if centre == ("-2", "0"):
        assert orbit.escaped and orbit.length == 1


def test_full_4096_view_at_1e_20_on_a_sample(gpu):
    mrd, span = 30000, 1e-20
    orbit = DeepOrbit(*SEAHORSE, mrd, min_span=span)
    view = DeepView(span, 4096)
    c, _, _, st = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
    pick = np.random.RandomState(11).choice(4096 * 4096, 4096, replace=False)
    zr, zi = orbit.table()
    dr, di = D.offsets(view)
    mc, _ = D.model_counts(zr, zi, dr[pick], di[pick], mrd)
    assert np.array_equal(c.ravel()[pick], mc), int((c.ravel()[pick] != mc).sum())
    assert len(np.unique(c)) >= 400 and st.pixel_iterations > 0


def test_bands_and_windows_equal_the_whole_view(gpu):
    mrd, span = 5000, 1e-20
    orbit = DeepOrbit(*SEAHORSE, mrd, min_span=span)
    view = DeepView(span, 200, 150)
    whole, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
    for window in [(0, 40, 200, 33), (13, 0, 101, 150), (199, 149, 1, 1), (64, 64, 8, 8)]:
        c0, r0, nc, nr = window
        part, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False)
        assert np.array_equal(part, whole[r0:r0 + nr, c0:c0 + nc]), window


def test_submit_torch_launch_and_render_equal_compute(gpu):
    import torch
    from distributedmandelbrot_amd.sharding import render_deep_view
    mrd, span = 5000, 1e-60
    orbit = DeepOrbit("0", "1", mrd, min_span=span)
    view = DeepView(span, 300, 260)
    c, b, _, _ = gpu.compute_deep_view(orbit, view, mrd)
    # submit / wait, two slots at once
    oc = [np.empty((130, 300), np.int32) for _ in range(2)]
    ob = [np.empty((130, 300), np.uint8) for _ in range(2)]
    for s in range(2):
        gpu.submit_deep_view(s, orbit, view, mrd, window=(0, 130 * s, 300, 130), out_counts=oc[s], out_bytes=ob[s])
    for s in range(2):
        gpu.wait(s)
    assert np.array_equal(np.vstack(oc), c) and np.array_equal(np.vstack(ob), b)
    # device pointers on a non-default torch stream
    stream = torch.cuda.Stream()
    dc = torch.full((260 * 300,), -5, dtype=torch.int32, device="cuda:0")
    db = torch.full((260 * 300,), 7, dtype=torch.uint8, device="cuda:0")
    ds = torch.zeros(260 * 300, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.data_ptr(), d_bytes=db.data_ptr(), d_smooth=ds.data_ptr(),
                             stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(dc.cpu().numpy().reshape(260, 300), c)
    assert np.array_equal(db.cpu().numpy().reshape(260, 300), b)
    # row bands of 128 over the devices of this process
    rc, rb, per = render_deep_view([gpu], orbit, view, mrd, band_rows=128)
    assert np.array_equal(rc, c) and np.array_equal(rb, b) and per[0]["bands"] == 3


def test_agrees_with_the_strict_path_at_1e_6(gpu):
    """Sanity: where binary64 still resolves the view, the deep path and the strict linspace path see the same picture (their
    coordinates differ by rounding only).  Measured (the numpy model and the C oracle, which the GPU equals): 99.22 % at mrd
    1000; 98.22 % at mrd 5000, where orbits are long enough for binary64's own rounding to decide boundary pixels -- on 40
    sampled pixels where the two differ, direct iteration at 256 bits agrees with the deep count 35 times, with the strict
    count 9 times."""
    mrd, span, n = 1000, 1e-6, 512
    orbit = DeepOrbit("-0.743643", "0.131825", mrd, min_span=span)
    deep, _, _, _ = gpu.compute_deep_view(orbit, DeepView(span, n), mrd, want_bytes=False)
    strict, _, _ = gpu.compute_view(View.centered(-0.743643, 0.131825, span, n), mrd, want_bytes=False)
    assert (deep == strict).mean() >= 0.99, float((deep == strict).mean())


def test_argument_errors(gpu):
    from distributedmandelbrot_amd import _lib as L
    orbit = DeepOrbit("0", "1", 1000, min_span=1e-20)
    view = DeepView(1e-20, 16)
    for bad_view in (DeepView(0.0, 16), DeepView(-1e-20, 16), DeepView(float("inf"), 16), DeepView(float("nan"), 16),
                     DeepView(2.0 ** -961, 16), DeepView(4.5, 16)):
        with pytest.raises(MbkError):
            gpu.compute_deep_view(orbit, bad_view, 100)
    gpu.compute_deep_view(orbit, DeepView(2.0 ** -960, 16), 100)      # the limits themselves are accepted
    gpu.compute_deep_view(orbit, DeepView(4.0, 16), 100)
    with pytest.raises(MbkError):
        gpu.compute_deep_view(orbit, view, 1001)                      # beyond the orbit's mrd
    with pytest.raises(MbkError):
        gpu.compute_deep_view(orbit, view, 100, window=(10, 0, 7, 16))
    with pytest.raises(MbkError):
        gpu.compute_deep_view(orbit, view, 100, want_counts=False, want_bytes=False)
    cv = gpu._cdeep(view, None)
    st = L.mbk_stats()
    out = np.empty(16 * 16, np.int32)
    for flags in (L.MBK_WANT_COUNTS | L.MBK_KERNEL_GROUP, L.MBK_WANT_COUNTS | L.MBK_PRECISION_F32,
                  L.MBK_WANT_COUNTS | L.MBK_LAZY_UNIFORM):
        assert gpu._lib.mbk_deep_view_compute(gpu._h, orbit._h, cv, 100, flags, out.ctypes.data, None, None, st) == L.MBK_ERR_INVALID
    assert gpu._lib.mbk_deep_view_compute(gpu._h, None, cv, 100, L.MBK_WANT_COUNTS, out.ctypes.data, None, None, st) == L.MBK_ERR_INVALID
    assert gpu._lib.mbk_deep_view_submit(gpu._h, 7, orbit._h, cv, 100, L.MBK_WANT_COUNTS, out.ctypes.data, None) == L.MBK_ERR_INVALID
    # the ctx still works afterwards
    c, _, _, _ = gpu.compute_deep_view(orbit, view, 100)
    assert c.shape == (16, 16)
