"""Deep-zoom views on the GPU (include/mbk.h, "Deep-zoom views"): the kernel is held bit for bit to the numpy restatement of
the contract (tests/deep_model.py) on the library's own orbit table, through every entry point."""
import numpy as np
import pytest

import deep_model as D
import smooth_truth as T
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
    # M = 1: the start state is rebased, and every step after it.  This holds the kernel to the model only; the picture
    # itself is wrong at the tip of the antenna (tests/test_deep_truth.py, the xfail cases): the model retires every pixel
    # at count 1 where direct iteration gives counts up to ~100.
    (("-2", "0"), 1e-60, (40, 24), 200, 1),
]


def _smooth_against_truth(sm, mc, mag, what, sample=4000):
    """The kernel's nu against the truth at (model count, model mag) -- the GPU's counts equal the model's, and so does
    the mag it took its logarithms of unless nu shows otherwise -- within A ulp(nu) + B 2^-52 (tests/smooth_truth.py) on
    every escaped pixel up to `sample`, a seeded sample beyond; and against numpy's evaluation on the whole array by the
    sum of the two bounds."""
    T.assert_pair(sm, D.smooth_from(mc, mag), mc, what)
    esc = np.flatnonzero(mc.ravel() > 0)
    if esc.size > sample:
        esc = np.random.RandomState(4).choice(esc, sample, replace=False)
    if esc.size:
        T.assert_within(sm.ravel()[esc], mc.ravel()[esc], mag.ravel()[esc], what)


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
    assert (sm[mc == 0] == 0.0).all()
    _smooth_against_truth(sm, mc, mag, f"deep {centre[0][:8]} {span:g}")
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


def test_launch_compute_and_submit_equal_the_model_on_a_ragged_window(gpu):
    """27 x 19 view, window (3, 2, 21, 13): partial 8 x 8 blocks on both edges and a nonzero origin; the orbit escapes at M = 58,
    so every pixel that runs on rebases (mrd 96).  The three forms, plain and with the bilinear approximation, bit for bit."""
    import torch
    mrd, window = 96, (3, 2, 21, 13)
    orbit = DeepOrbit("1e-21", "1", mrd, min_span=1e-20)
    assert orbit.escaped and orbit.length == 58
    view = DeepView(1e-20, 27, 19)
    mc, _ = _model(orbit, view, mrd, window)
    assert mc.max() > orbit.length and len(np.unique(mc)) >= 8
    exact = None
    for bla in (False, True):
        c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, window=window, want_smooth=True, bla=bla)
        if not bla:
            assert np.array_equal(c, mc) and np.array_equal(b, _bytes(mc, mrd))
            exact = c
        else:
            assert (c == exact).mean() >= 0.99
        sc, sb = np.full((13, 21), -7, np.int32), np.full((13, 21), 0xA5, np.uint8)
        gpu.submit_deep_view(3, orbit, view, mrd, window=window, out_counts=sc, out_bytes=sb, bla=bla)
        sst = gpu.wait(3)
        assert np.array_equal(sc, c) and np.array_equal(sb, b)
        assert (sst.pixel_iterations, sst.never_pixels, sst.rle_runs) == (st.pixel_iterations, st.never_pixels, st.rle_runs)
        px = 13 * 21
        dc = torch.full((px + 32,), -7, dtype=torch.int32, device="cuda:0")
        db = torch.full((px + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
        ds = torch.full((px + 32,), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        gpu.launch_deep_view(orbit, view, mrd, window=window, d_counts=dc.data_ptr() + 64, d_bytes=db.data_ptr() + 16,
                             d_smooth=ds.data_ptr() + 128, bla=bla)
        torch.cuda.synchronize()
        gc, gb, gs = dc.cpu().numpy(), db.cpu().numpy(), ds.cpu().numpy()
        assert np.array_equal(gc[16:16 + px].reshape(13, 21), c) and (gc[:16] == -7).all() and (gc[16 + px:] == -7).all()
        assert np.array_equal(gb[16:16 + px].reshape(13, 21), b) and (gb[:16] == 0xA5).all() and (gb[16 + px:] == 0xA5).all()
        assert np.array_equal(gs[16:16 + px].reshape(13, 21).view(np.uint64), sm.view(np.uint64))
        assert (gs[:16] == -7.0).all() and (gs[16 + px:] == -7.0).all()


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


def _bytes(counts, mrd):
    """ceil(count * 256 / mrd) mod 256 in exact integers."""
    return ((counts.astype(np.int64) * 256 + mrd - 1) // mrd % 256).astype(np.uint8)


def _check(gpu, orbit, view, mrd, window=None, smooth=True):
    """compute_deep_view against the model: counts, bytes, smooth, statistics.  Returns the counts."""
    c, b, sm, st = gpu.compute_deep_view(orbit, view, mrd, window=window, want_smooth=smooth)
    mc, mag = _model(orbit, view, mrd, window)
    assert np.array_equal(c, mc), (mrd, window, int((c != mc).sum()))
    assert np.array_equal(b, _bytes(mc, mrd)), (mrd, window)
    if smooth:
        assert (sm[mc == 0] == 0.0).all()
        _smooth_against_truth(sm, mc, mag, f"deep mrd {mrd} window {window}")
    assert st.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum()), mrd
    assert st.never_pixels == int((c == 0).sum())
    return c


@pytest.mark.parametrize("centre, span, orbit_mrd", [(("1e-21", "1"), 1e-20, 5000), (("0", "1"), 1e-30, 3000)])
def test_launch_mrd_below_and_around_the_orbit_length(gpu, centre, span, orbit_mrd):
    """A launch's mrd, not the orbit's, bounds the loop: 1, 2, 3, 100, M - 1, M, M + 1 and the orbit's mrd, on an orbit
    that escapes at M = 58 and on one that does not escape (M = its mrd)."""
    orbit = DeepOrbit(*centre, orbit_mrd, min_span=span)
    M = orbit.length
    assert (M, orbit.escaped) == ((58, True) if centre[0] == "1e-21" else (orbit_mrd, False))
    view = DeepView(span, 40, 36)
    seen = set()
    for mrd in sorted({1, 2, 3, 100, M - 1, M, M + 1, orbit_mrd} & set(range(1, orbit_mrd + 1))):
        c = _check(gpu, orbit, view, mrd)
        seen.add(len(np.unique(c)))
    assert max(seen) >= 8
    with pytest.raises(MbkError):
        gpu.compute_deep_view(orbit, view, orbit_mrd + 1)
    c, b, _, _ = gpu.compute_deep_view(orbit, view, 0, want_bytes=False)
    assert b is None and c.shape == (36, 40) and not c.any()


@pytest.mark.parametrize("centre, span, M", [(("0.3", "0"), 0.3, 12), (("-2", "0"), 1.0, 1)])
def test_short_orbit_rebases_at_its_end(gpu, centre, span, M):
    """The reference escapes within a few steps while most pixels of the view never do: they run off the end of the orbit
    (m == M) again and again and must rebase there each time."""
    mrd = 2000
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    assert orbit.escaped and orbit.length == M
    c = _check(gpu, orbit, DeepView(span, 64, 48), mrd)
    assert (c == 0).any() and (c > M + 1).sum() > 100 and len(np.unique(c)) >= 15


@pytest.mark.parametrize("span", [2.0 ** -960, 2.0 ** -900], ids=["2^-960", "2^-900"])
def test_deepest_spans_through_subnormal_offsets(gpu, span):
    """At the deepest spans dz starts near 2^-970 and |dz|^2 underflows; as dz grows, |dz|^2 passes through the binary64
    subnormal range, where a device that flushed f64 denormals would rebase (or not) differently."""
    mrd = 3000
    orbit = DeepOrbit("0", "1", mrd, min_span=span)
    view = DeepView(span, 24, 20, span)             # square pixels would make span_i < 2^-960
    c = _check(gpu, orbit, view, mrd)
    assert len(np.unique(c)) >= 8 and (c > 0).all()
    sub = [0]

    def on_step(dr, di):
        d2 = dr * dr + di * di
        sub[0] += int(((d2 > 0.0) & (d2 < 2.0 ** -1022)).sum())

    zr, zi = orbit.table()
    dr, di = D.offsets(view)
    D.model_counts(zr, zi, dr, di, mrd, on_step=on_step)
    assert sub[0] >= view.width * view.height, sub[0]     # every pixel, at least once


def test_widest_span(gpu):
    orbit = DeepOrbit("-0.5", "0", 400, min_span=4.0)
    c = _check(gpu, orbit, DeepView(4.0, 64, 56), 400)
    assert len(np.unique(c)) >= 20 and (c == 0).any()


@pytest.mark.parametrize("view, window", [
    (DeepView(1e-30, 1), None),
    (DeepView(1e-30, 1, 64), None),
    (DeepView(1e-30, 64, 1), None),
    (DeepView(1e-30, 7, 9), None),
    (DeepView(1e-30, 65, 17), None),
    (DeepView(1e-30, 50, 30, 3e-30), None),         # pixels 2.04e-32 wide, 1.03e-31 high
    (DeepView(1e-30, 100, 70), (3, 5, 17, 11)),
    (DeepView(1e-30, 100, 70), (61, 1, 39, 69)),
    (DeepView(1e-30, 100, 70), (0, 69, 100, 1)),
    (DeepView(1e-30, 100, 70), (99, 0, 1, 70)),
    (DeepView(1e-30, 100, 70, 4e-31), (9, 13, 83, 50)),
], ids=["1x1", "1x64", "64x1", "7x9", "65x17", "span_i", "win-3-5", "win-61-1", "win-last-row", "win-last-col",
        "win-span_i"])
def test_view_shapes_and_windows(gpu, view, window):
    """Views that are not multiples of the 8x8 block, single rows and columns, non-square pixels, and windows that start
    and end off the block grid (the offsets use the view's width and height, not the window's)."""
    mrd = 3000
    orbit = DeepOrbit("0", "1", mrd, min_span=1e-30)
    c = _check(gpu, orbit, view, mrd, window)
    if window is None and c.size > 1:
        assert len(np.unique(c)) >= 8
    if window is not None:
        whole = _check(gpu, orbit, view, mrd, smooth=False)
        assert len(np.unique(whole)) >= 20
        c0, r0, nc, nr = window
        assert np.array_equal(c, whole[r0:r0 + nr, c0:c0 + nc])


@pytest.mark.parametrize("mrd", [2 ** 24 + 3, 2 ** 31 - 1])
def test_wide_quantiser(gpu, mrd):
    """mrd >= 2^23 takes the 64-bit quantiser (quant_wide).  Centre 1.5 + 1.5i: the orbit escapes at M = 1, and every pixel
    of the view (real parts >= 0.5, outside the set) within a few steps, so a huge mrd is cheap."""
    from oracle.oracle import numpy_quantise
    orbit = DeepOrbit("1.5", "1.5", mrd, min_span=1e-3)
    assert orbit.escaped and orbit.length == 1
    view = DeepView(2.0, 48, 40)
    c = _check(gpu, orbit, view, mrd)
    assert (c > 0).all() and len(np.unique(c)) >= 3
    _, b, _, _ = gpu.compute_deep_view(orbit, view, mrd, want_counts=False)
    assert np.array_equal(b, numpy_quantise(c, mrd)) and (b == 1).all()


def test_smooth_on_a_window_and_through_launch(gpu):
    import torch
    mrd, span = 5000, 1e-20
    orbit = DeepOrbit("1e-21", "1", mrd, min_span=span)
    view = DeepView(span, 90, 60)
    window = (5, 7, 70, 41)
    _check(gpu, orbit, view, mrd, window)
    _, _, sm, _ = gpu.compute_deep_view(orbit, view, mrd, want_smooth=True)
    mc, mag = _model(orbit, view, mrd)
    for with_counts in (False, True):
        dc = torch.full((60 * 90,), -5, dtype=torch.int32, device="cuda:0")
        ds = torch.full((60 * 90,), -1.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.data_ptr() if with_counts else 0, d_smooth=ds.data_ptr())
        torch.cuda.synchronize()
        got = ds.cpu().numpy().reshape(60, 90)
        assert np.array_equal(got, sm)          # the same kernel, bit for bit
        _smooth_against_truth(got, mc, mag, f"deep launch counts={with_counts}")
        assert np.array_equal(dc.cpu().numpy().reshape(60, 90), mc if with_counts else np.full_like(mc, -5))


@pytest.mark.parametrize("case", T.DEEP_CASES[7:], ids=["span-2^-960", "span-4", "M-1"])
def test_smooth_at_the_deepest_and_widest_span_and_on_a_one_step_orbit(gpu, case):
    """nu against the truth at span 2^-960 (|dz|^2 subnormal for most of the run), at span 4, and on the M == 1 orbit of
    centre -2, where the escaping |z|^2 comes from a state that was rebased every step."""
    orbit, view, mrd, window, mc, mag = T.deep_model_case(case)
    c, _, sm, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, want_smooth=True)
    assert np.array_equal(c, mc)
    assert (sm[mc == 0] == 0.0).all() and (mc > 0).sum() >= 400 and len(np.unique(mc)) >= 8
    _smooth_against_truth(sm, mc, mag, f"deep {case[0][0]} span {case[1]:g}")
    if case[0] == ("-2", "0"):
        assert orbit.length == 1 and orbit.escaped


def _cusp_orbit(k, mrd):
    """Orbits of equal length (mrd: the centres lie inside the cardioid) whose pictures differ: centre 0.25 - k 2^-19 on the
    real axis, views that reach past the cusp at 0.25."""
    return DeepOrbit("%.20f" % (0.25 - k * 2.0 ** -19), "0", mrd, min_span=1e-30)


CUSP_VIEW = DeepView(1e-4, 48, 8, 1e-30)


def test_orbit_copies_rotate_through_the_cache(gpu):
    """12 orbits in rotation on one ctx (8 device copies at most): each result is its own orbit's picture."""
    mrd = 1500
    orbits = [DeepOrbit("%de-22" % (3 * k + 1), "1", mrd, min_span=1e-20) for k in range(12)]
    view = DeepView(1e-20, 32, 24)
    models = [_model(o, view, mrd)[0] for o in orbits]
    assert len({m.tobytes() for m in models}) == 12
    for order in (range(12), reversed(range(12)), [0, 9, 1, 10, 2, 11, 3, 0, 9]):
        for k in order:
            c, _, _, _ = gpu.compute_deep_view(orbits[k], view, mrd, want_bytes=False)
            assert np.array_equal(c, models[k]), k


def test_eviction_waits_for_launches_in_flight():
    """Slots 1-3 hold submitted launches of cached copies when a ninth orbit makes the ctx free every copy: the launches
    in flight still read their own orbits."""
    from distributedmandelbrot_amd import MandelbrotDevice
    mrd = 3000
    orbits = [_cusp_orbit(k, mrd) for k in range(9)]
    view = DeepView(1e-4, 256, 64, 1e-30)
    models = [_model(o, view, mrd)[0] for o in orbits]
    assert len({m.tobytes() for m in models}) == 9
    with MandelbrotDevice(0) as dev:
        for o in orbits[:8]:
            dev.compute_deep_view(o, CUSP_VIEW, mrd, want_bytes=False)      # 8 copies: the cache is full
        out = {s: np.empty((64, 256), np.int32) for s in (1, 2, 3)}
        for s in (1, 2, 3):
            dev.submit_deep_view(s, orbits[4 + s], view, mrd, out_counts=out[s])
        c, _, _, _ = dev.compute_deep_view(orbits[8], view, mrd, want_bytes=False)   # the ninth: evicts all eight
        for s in (1, 2, 3):
            dev.wait(s)
            assert np.array_equal(out[s], models[4 + s]), s
        assert np.array_equal(c, models[8])
        for k in (7, 0, 8):                                                # re-uploaded after the eviction
            c, _, _, _ = dev.compute_deep_view(orbits[k], view, mrd, want_bytes=False)
            assert np.array_equal(c, models[k]), k


def test_destroyed_orbits_never_alias_new_ones(gpu):
    """Destroy an orbit, create the next (the allocator may hand it the same host address), launch: the ctx must not take
    the dead orbit's device copy for the new one.  The orbits have equal length."""
    mrd = 2000
    for k in range(10):
        orbit = _cusp_orbit(k, mrd)
        assert orbit.length == mrd and not orbit.escaped
        mc = _model(orbit, CUSP_VIEW, mrd)[0]
        c, _, _, _ = gpu.compute_deep_view(orbit, CUSP_VIEW, mrd, want_bytes=False)
        assert np.array_equal(c, mc), k
        orbit.close()


def test_one_orbit_on_two_contexts(gpu):
    from distributedmandelbrot_amd import MandelbrotDevice
    mrd = 3000
    orbit = _cusp_orbit(2, mrd)
    mc = _model(orbit, CUSP_VIEW, mrd)[0]
    with MandelbrotDevice(0) as other:
        a, _, _, _ = other.compute_deep_view(orbit, CUSP_VIEW, mrd, want_bytes=False)
        b, _, _, _ = gpu.compute_deep_view(orbit, CUSP_VIEW, mrd, want_bytes=False)
        a2, _, _, _ = other.compute_deep_view(orbit, CUSP_VIEW, mrd, want_bytes=False)
        assert np.array_equal(a, mc) and np.array_equal(b, mc) and np.array_equal(a2, mc)
    c, _, _, _ = gpu.compute_deep_view(orbit, CUSP_VIEW, mrd, want_bytes=False)   # the other ctx's copy is gone, not this one
    assert np.array_equal(c, mc)
