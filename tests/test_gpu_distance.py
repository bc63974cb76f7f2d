"""Exterior distance estimates on the GPU (include/mbk.h, "Distance estimates"), held to the numpy model of the contract
(tests/distance_model.py) and to the truth of the output expression.

The counts are compared with compute_view's bit for bit.  The states behind de (z, d, mag, dmag) are exact in the model, so
the device's de must be the model's value wherever ocml's ln and numpy's agree, and elsewhere the value a neighbouring ln
gives (distance_model.assert_states_agree: one of the candidates matches every sample, which no wrong state survives); and
every sample is within D_GPU = D0 + 1 ulp(de) of the correctly rounded expression at the model's (mag, dmag).
Both designs run everywhere: kernel "asm" is the one-pass form, the other selectors the two-pass form.

Measured on gfx950 (ocml, ROCm 7): every sample of every small case equals the numpy model bit for bit, with every kernel, cycle
test on and off; of 20 000 seeded escaped pixels of cfg5 99.98 % do and the rest are a neighbouring ln's value; worst 1.953
ulp(de) against the correctly rounded expression (n = 37, mag = 1578374554315972.8, dmag = 9.698205231076945e+24; allowed 2.95),
on the small cases 1.941 at the pixel and to the digits of glibc.  Koebe lines: tip 3.885412 .. 3.999993, cusp 0.001837 ..
0.599069, neck <= 0.028517, the CPU model's figures.
"""
import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

import distance_model as M
import smooth_truth as T
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import resolve_host

pytestmark = pytest.mark.gpu

KERNELS = ["default", "asm", "group", "scan"]          # the selectors smooth accepts
_MODEL = {}


def _model(case):
    name, v, mrd, window = case
    if name not in _MODEL:
        _MODEL[name] = M.model(v, mrd, window)
    return _MODEL[name]


@pytest.fixture(scope="module")
def strict():
    """A second ctx with the cycle test off."""
    from distributedmandelbrot_amd import MandelbrotDevice
    with MandelbrotDevice(0) as dev:
        dev.set_option("cycle_detect", 0)
        yield dev


@pytest.mark.parametrize("cycle", [1, 0], ids=["cycle", "strict"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_small_views_every_sample(gpu, strict, kernel, cycle):
    """Ragged sizes, windows, step-zero axes, tiny imaginary parts (the literal-doubling path), the |c| = 2 ring with c = -2
    itself, |c| up to 74, and magnitudes up to and past the binary64 overflow."""
    dev = gpu if cycle else strict
    assert dev.get_option("cycle_detect") == cycle
    for case in T.SMALL_CASES:
        name, v, mrd, window = case
        what = f"{name} {kernel} cycle={cycle}"
        mde, mn, st = _model(case)
        counts, _, _ = dev.compute_view(View(*v), mrd, window=window, want_bytes=False)
        de, c, stats = dev.compute_view_distance(View(*v), mrd, window=window, kernel=kernel)
        assert de.shape == c.shape == mn.shape and de.dtype == np.float64 and c.dtype == np.int32
        assert np.array_equal(c, counts), (what, int((c != counts).sum()))
        assert np.array_equal(c, mn), (what, int((c != mn).sum()))
        assert not np.isnan(de).any() and (de[c == 0] == 0.0).all() and (de >= 0.0).all(), what
        share = M.assert_states_agree(de, st, what)
        print(f"{what}: {100 * share:.2f} % of the samples equal the numpy model bit for bit")
        M.assert_expression_within(de, st, what, M.D_GPU)
        assert stats.pixel_iterations == int(np.where(c > 0, c, max(mrd - 1, 0)).astype(np.int64).sum()), what
        assert stats.never_pixels == int((c == 0).sum()), what
        if name == "ring":          # c = -2 + 0i: z stays at 2 through all 64 run-on steps, d_k = (4^(k+1) - 1) / 3
            assert c[16, 0] == 1 and st["extra"].reshape(c.shape)[16, 0] == M.RUN_ON
            assert 0.0 < de[16, 0] < 1e-30
        if name == "huge":
            assert np.isinf(de).any() and np.isfinite(de).any() and (de[np.isinf(st["mag"]).reshape(c.shape)] == math.inf).all()
        if name == "2^499":
            assert (de == math.inf).all()


BIG = (View(-2.0, -1.5, 3.0, 3.0, 2048, 2048), 500)
BIG_WINDOWS = [(0, 1000, 2048, 8), (0, 1021, 2048, 3), (0, 2045, 2048, 3), (300, 700, 513, 129), (2047, 2047, 1, 1),
               (13, 0, 1, 2048), (1023, 1023, 2, 2)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_window_equals_the_same_pixels_of_the_whole_view(gpu, kernel):
    view, mrd = BIG
    whole, wc, wst = gpu.compute_view_distance(view, mrd, kernel=kernel)
    ref, _, _ = gpu.compute_view(view, mrd, want_bytes=False)
    assert np.array_equal(wc, ref) and len(np.unique(wc)) >= 100 and (wc == 0).any()
    assert np.array_equal(whole == 0.0, wc == 0) and np.isfinite(whole).all()
    for window in BIG_WINDOWS:
        c0, r0, nc, nr = window
        de, c, st = gpu.compute_view_distance(view, mrd, window=window, kernel=kernel)
        assert np.array_equal(c, wc[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(de, whole[r0:r0 + nr, c0:c0 + nc]), window
        assert st.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum()), window
    if kernel != "default":      # the two designs store the same values
        other, _, _ = gpu.compute_view_distance(view, mrd)
        assert np.array_equal(other, whole)


def _device_buffers(torch, px, guard):
    dd = torch.full((px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    return dd, dc


@pytest.mark.parametrize("kernel", KERNELS)
def test_launch_view_distance_on_a_torch_stream(gpu, kernel):
    """Device pointers, the caller's stream, with and without d_counts: the same values as compute_view_distance, and the
    guard regions in front of and behind the window-sized buffers keep their sentinels."""
    import torch
    view, mrd = View(-2.0, -1.5, 3.0, 3.0, 600, 400), 700
    guard = 1024
    stream = torch.cuda.Stream(device="cuda:0")
    whole_de, whole_c, _ = gpu.compute_view_distance(view, mrd, kernel=kernel)
    for window in (None, (37, 101, 333, 77), (0, 200, 600, 8), (599, 399, 1, 1)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        want_de, want_c = whole_de[r0:r0 + nr, c0:c0 + nc], whole_c[r0:r0 + nr, c0:c0 + nc]
        px = want_de.size
        bufs = [_device_buffers(torch, px, guard) for _ in range(2)]
        torch.cuda.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            gpu.launch_view_distance(view, mrd, d_distance=dd[guard:].data_ptr(), d_counts=dc[guard:].data_ptr() if with_counts else 0,
                                     stream=stream.cuda_stream, window=window, kernel=kernel)
        stream.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            hd, hc = dd.cpu().numpy(), dc.cpu().numpy()
            assert np.array_equal(hd[guard:guard + px].reshape(want_de.shape), want_de), (window, with_counts)
            assert (hd[:guard] == -77.0).all() and (hd[guard + px:] == -77.0).all(), (window, with_counts)
            assert (hc[:guard] == -5).all() and (hc[guard + px:] == -5).all(), (window, with_counts)
            if with_counts:
                assert np.array_equal(hc[guard:guard + px].reshape(want_c.shape), want_c), window
            else:
                assert (hc == -5).all(), window


def test_argument_errors_write_nothing_and_shallow_mrd(gpu):
    import torch
    view = View(-2.0, -2.0, 4.0, 4.0, 16, 16)
    cv = gpu._cview(view, None)
    guard = 64
    dd, dc = _device_buffers(torch, 256, guard)
    torch.cuda.synchronize()
    pd, pc = dd[guard:].data_ptr(), dc[guard:].data_ptr()
    launch = gpu._lib.mbk_view_launch_distance
    with pytest.raises(MbkError):
        gpu.launch_view_distance(view, 100, d_distance=0, d_counts=pc)
    assert launch(gpu._h, C.byref(cv), 100, L.MBK_KERNEL_DEFAULT, pc, None, None) == L.MBK_ERR_INVALID
    for kernel in KERNELS:
        assert launch(gpu._h, C.byref(cv), 100, L.KERNELS[kernel] | L.MBK_PRECISION_F32, pc, pd, None) == L.MBK_ERR_INVALID
    for kernel in ("simple", "refill"):
        with pytest.raises(MbkError):
            gpu.launch_view_distance(view, 100, d_distance=pd, d_counts=pc, kernel=kernel)
        with pytest.raises(MbkError):
            gpu.compute_view_distance(view, 100, kernel=kernel)
    assert launch(gpu._h, C.byref(cv), 100, 0x600, pc, pd, None) == L.MBK_ERR_INVALID          # unknown selector
    with pytest.raises(MbkError):
        gpu.launch_view_distance(view, 2 ** 31, d_distance=pd)
    with pytest.raises(MbkError):
        gpu.launch_view_distance(view, 100, d_distance=pd, window=(10, 0, 7, 16))
    with pytest.raises(MbkError):
        gpu.launch_view_distance(View(2.0 ** 500, 0.0, 2.0 ** 500, 1.0, 4, 4), 100, d_distance=pd)
    assert launch(gpu._h, None, 100, L.MBK_KERNEL_DEFAULT, None, pd, None) == L.MBK_ERR_INVALID
    h = np.full(256, -1.0)
    assert gpu._lib.mbk_view_compute_distance(gpu._h, C.byref(cv), 100, 0, None, None, None) == L.MBK_ERR_INVALID
    assert gpu._lib.mbk_view_compute_distance(gpu._h, None, 100, 0, None, h.ctypes.data, None) == L.MBK_ERR_INVALID
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all() and (h == -1.0).all()
    for mrd in (0, 1, 2):
        for kernel in KERNELS:
            dd, dc = _device_buffers(torch, 256, guard)
            torch.cuda.synchronize()
            gpu.launch_view_distance(view, mrd, d_distance=dd[guard:].data_ptr(), d_counts=dc[guard:].data_ptr(), kernel=kernel)
            torch.cuda.synchronize()
            hd, hc = dd.cpu().numpy(), dc.cpu().numpy()
            assert (hd[:guard] == -77.0).all() and (hd[guard + 256:] == -77.0).all()
            assert (hc[:guard] == -5).all() and (hc[guard + 256:] == -5).all()
            de, c, st = gpu.compute_view_distance(view, mrd, kernel=kernel)
            assert np.array_equal(hd[guard:guard + 256].reshape(16, 16), de) and np.array_equal(hc[guard:guard + 256].reshape(16, 16), c)
            if mrd < 2:
                assert not de.any() and not c.any() and st.pixel_iterations == 0 and st.never_pixels == 256
            else:
                mde, mn, mst = M.model((-2.0, -2.0, 4.0, 4.0, 16, 16), 2)
                assert np.array_equal(c, mn) and set(np.unique(c)) == {0, 1}
                M.assert_states_agree(de, mst, f"mrd 2 {kernel}")


@pytest.mark.parametrize("kernel", ["default", "asm"])
def test_cfg5_full_size(gpu, kernel):
    """cfg5's view at 4096^2, mrd 5000: the counts are compute_view's (and hash to tests/golden/bench_outputs.json), de is
    finite and >= 0 everywhere and 0 exactly where the count is 0, and a seeded sample of 20 000 escaped pixels is held to the
    model and to the truth of the expression."""
    (v, mrd) = T.CFG5
    view = View(*v)
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bench_outputs.json")))["cfg5"]
    assert g["view"] == list(v) and g["mrd"] == mrd
    de, c, st = gpu.compute_view_distance(view, mrd, kernel=kernel)
    ref, _, _ = gpu.compute_view(view, mrd, want_bytes=False)
    assert np.array_equal(c, ref)
    assert hashlib.sha256(c.tobytes()).hexdigest() == g["counts_sha256"]
    assert st.pixel_iterations == g["pixel_iterations"] and st.never_pixels == g["never_pixels"]
    assert np.isfinite(de).all() and (de >= 0.0).all()
    assert np.array_equal(de == 0.0, c == 0)
    esc = np.flatnonzero(c.ravel() > 0)
    pick = np.sort(np.random.RandomState(5).choice(esc, 20000, replace=False))
    cr, ci = M.axes(v)
    mst = M.states(cr[pick % view.width], ci[pick // view.width], mrd)
    assert np.array_equal(mst["n"], c.ravel()[pick])
    share = M.assert_states_agree(de.ravel()[pick], mst, f"cfg5 {kernel}")
    print(f"cfg5 {kernel}: {100 * share:.2f} % of 20 000 samples equal the numpy model bit for bit")
    M.assert_expression_within(de.ravel()[pick], mst, f"cfg5 {kernel}", M.D_GPU)


TS = np.logspace(-6, -1, 300)
KOEBE = 4.0 * (1.0 + 2.0 ** -10)


def _gpu_line(gpu, cr, ci, mrd, kernel):
    """The samples (cr[k], ci[k]) as 1 x 1 views (a view is a linspace; the lines are log-spaced)."""
    de = np.empty(cr.size)
    for k in range(cr.size):
        d, c, _ = gpu.compute_view_distance(View(float(cr[k]), float(ci[k]), 0.0, 0.0, 1, 1), mrd, kernel=kernel)
        assert c[0, 0] > 0, (k, "mrd too small")
        de[k] = d[0, 0]
    return de


@pytest.mark.parametrize("kernel", ["default", "asm"])
def test_koebe_bounds_on_gpu_output(gpu, kernel):
    """The three lines of tests/test_distance.py on the device's own output: de <= 4 |c - m| (1 + 2^-10) for m in the set,
    and de >= 3.8 t on the antenna tip."""
    cr = -2.0 - TS
    de = _gpu_line(gpu, cr, np.zeros_like(cr), 1000, kernel)
    dist = np.abs(cr + 2.0)
    print(f"tip {kernel}: de / distance in [{(de / dist).min():.6f}, {(de / dist).max():.6f}]")
    assert (de <= KOEBE * dist).all() and (de >= 3.8 * dist).all()
    cr = 0.25 + TS
    de = _gpu_line(gpu, cr, np.zeros_like(cr), 100000, kernel)
    dist = np.abs(cr - 0.25)
    print(f"cusp {kernel}: de / distance in [{(de / dist).min():.6f}, {(de / dist).max():.6f}]")
    assert (de > 0).all() and (de <= KOEBE * dist).all()
    de = _gpu_line(gpu, np.full_like(TS, -0.75), TS, 3_300_000, kernel)
    print(f"neck {kernel}: de / distance in [{(de / TS).min():.6f}, {(de / TS).max():.6f}]")
    assert (de > 0).all() and (de <= KOEBE * TS).all()


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


@pytest.mark.parametrize("kernel", ["default", "asm"])
@pytest.mark.parametrize("s", [1, 2, 4])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s, kernel):
    """render_view(source="distance") is mbk_render_resolve_host (held to the numpy rule by tests/test_distance.py) of the
    samples compute_view_distance returns for the s times finer view, banded and unbanded, whole and windowed."""
    w, h = (509, 383) if s < 4 else (253, 189)
    span = 0.2
    view, mrd = View(-0.1 - span / 2, 0.65 - span / 2 * h / w, span, span * h / w, w, h), 400
    pal = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 255)).for_distance(view, 12.0)
    de, counts, st_s = gpu.compute_view_distance(_finer(view, s), mrd, kernel=kernel)
    assert len(np.unique(counts)) > 10 and (counts == 0).any()
    want = resolve_host(pal, "distance", s, w, h, counts=counts, smooth=de)
    want_model = M.render_distance(pal.entries, pal.inside, pal.scale, pal.offset, s, counts, de)
    assert np.array_equal(want, want_model)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    for rows in (0, 1, 37):
        img, st = gpu.render_view(view, mrd, palette=pal, source="distance", supersample=s, kernel=kernel, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (100, 50, 77, 53)
    img, _ = gpu.render_view(view, mrd, palette=pal, source="distance", supersample=s, kernel=kernel, window=window)
    assert np.array_equal(img, want[50:103, 100:177])
    if s == 1:
        import torch
        d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
        gpu.launch_render_view(view, mrd, palette=pal, d_rgba=d.data_ptr(), source="distance", supersample=s, kernel=kernel)
        torch.cuda.synchronize()
        hd = d.cpu().numpy()
        assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


def test_render_refusals(gpu):
    view = View(-2.0, -1.5, 3.0, 3.0, 64, 64)
    pal = Palette.distance(view, 8.0)
    for kernel in ("simple", "refill"):
        with pytest.raises(MbkError):
            gpu.render_view(view, 100, palette=pal, source="distance", kernel=kernel)
    spec = pal.spec("distance", 1)
    out = np.full((64, 64, 4), 7, np.uint8)
    cv = gpu._cview(view, None)
    assert gpu._lib.mbk_view_render_compute(gpu._h, C.byref(cv), 100, L.MBK_PRECISION_F32, C.byref(spec), out.ctypes.data,
                                            None) == L.MBK_ERR_INVALID
    for bad in (Palette(pal.entries, scale=2.0 ** 81), Palette(pal.entries, scale=0.0), Palette(pal.entries[:1])):
        with pytest.raises(MbkError):
            gpu.render_view(view, 100, palette=bad, source="distance")
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    with pytest.raises(MbkError) as e:
        gpu.render_deep_view(orbit, DeepView(1e-20, 32, 32), 500, palette=pal, source="distance")
    assert "plain views only" in str(e.value)
    assert (out == 7).all()
    img, _ = gpu.render_view(view, 100, palette=Palette(pal.entries, scale=2.0 ** 80), source="distance")
    assert img.shape == (64, 64, 4)


def test_distance_render_marks_filaments_that_no_sample_hits(gpu):
    """The point of the feature.  A 256 x 256 view of the antenna left of the period-3 copy, [-1.785, -1.735] x [-0.005, 0.045],
    mrd 2000, pitch 0.05 / 255.  Chosen with the numpy model on the CPU: 10 189 samples never escape (the copy at -1.7549 and
    the real axis' neighbourhood), and 145 rows more than 4 pitches away from the real axis hold NO never-escaping sample at
    s = 1 although filaments cross them: 965 of their samples have de < pitch -- the set passes within a pixel of them, and an
    escape-time picture of those rows shows no trace of it.  The distance render paints them."""
    v, mrd = (-1.785, -0.005000000000000001, 0.05, 0.05, 256, 256), 2000
    view = View(*v)
    pitch = 0.05 / 255
    de, c, _ = gpu.compute_view_distance(view, mrd)
    mde, mn, _ = M.model(v, mrd)
    assert np.array_equal(c, mn) and int((c == 0).sum()) == 10189
    ys = np.linspace(v[1], v[1] + v[3], 256)
    rows = [r for r in range(256) if (c[r] > 0).all() and (de[r] < pitch).any() and abs(ys[r]) > 4 * pitch]
    mrows = [r for r in range(256) if (mn[r] > 0).all() and (mde[r] < pitch).any() and abs(ys[r]) > 4 * pitch]
    assert rows == mrows and len(rows) == 145 and int((de[rows] < pitch).sum()) == 965
    # black within one pixel of the set, white beyond two; the inside in red so that a hit sample would show
    pal = Palette.distance(view, 2.0, inner_px=1.0, inside=(255, 0, 0, 255))
    img, _ = gpu.render_view(view, mrd, palette=pal, source="distance")
    for r in rows:
        black = (img[r, :, :3] == 0).all(axis=1)
        red = (img[r, :, 0] == 255) & (img[r, :, 1] == 0)
        assert black[de[r] <= pitch].all() and black.any() and not red.any(), r       # marked, and no inside sample
        assert (img[r, de[r] >= 2 * pitch, :3] == 255).all(), r
