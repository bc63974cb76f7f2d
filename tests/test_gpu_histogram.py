"""Count histograms and histogram-equalised renders on the GPU (include/mbk.h, "Count histograms and histogram-equalised
colouring"): the device's tables are held exactly to np.bincount of the counts the same device returns, the renders byte for
byte to the numpy restatement of the contract (tests/histogram_model.py) applied to the device's own samples, and every refusal
leaves its output untouched."""
import ctypes as C

import numpy as np
import pytest

import histogram_model as H
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import equalize_lut

pytestmark = pytest.mark.gpu

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
GUARD = 0x5A5A5A5A5A5A5A5A
EQ_PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255)).for_equalized()


def _torch():
    import torch
    return torch


def _device_hist(gpu, counts, mrd, *, calls=1, offset=0):
    """counts_histogram of a host array through device buffers: the table with 16 guard words on either side, after `calls`
    accumulating calls.  offset: elements by which the counts buffer is shifted off its 16-byte alignment."""
    torch = _torch()
    c = torch.from_numpy(np.concatenate([np.zeros(offset, np.int32), np.ascontiguousarray(counts, np.int32).ravel()])).to("cuda:0")
    buf = torch.from_numpy(np.full(mrd + 32, GUARD, np.uint64).view(np.int64)).to("cuda:0")
    buf[16:16 + mrd] = 0
    torch.cuda.synchronize()
    for _ in range(calls):
        gpu.counts_histogram(c.data_ptr() + 4 * offset, counts.size, mrd, buf.data_ptr() + 8 * 16)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[:16] == GUARD).all() and (got[16 + mrd:] == GUARD).all(), "guard words changed"
    return got[16:16 + mrd]


@pytest.mark.parametrize("mrd", [30000, 1 << 20])
def test_random_counts_equal_bincount(gpu, mrd):
    rs = np.random.RandomState(21)
    for n, offset in [(1 << 22, 0), (1000003, 1), (5, 3), (1, 0), (2051, 2)]:
        counts = rs.randint(0, mrd, n).astype(np.int32)
        assert np.array_equal(_device_hist(gpu, counts, mrd, offset=offset), H.histogram(counts, mrd)), (n, offset)


def test_one_value_buffers_and_accumulation(gpu):
    for value, mrd in [(0, 1000), (1, 1000), (999, 1000), (25000, 30000), ((1 << 20) - 1, 1 << 20)]:
        counts = np.full(3 * 1024 * 1024 + 7, value, np.int32)
        got = _device_hist(gpu, counts, mrd)
        assert got[value] == counts.size and got.sum() == counts.size, value
    rs = np.random.RandomState(22)
    counts = rs.randint(0, 5000, 700001).astype(np.int32)
    assert np.array_equal(_device_hist(gpu, counts, 5000, calls=2), 2 * H.histogram(counts, 5000))
    # coherent data: long runs of a few values around a block of zeros, a window far from 0
    runs = np.repeat(rs.randint(20000, 20400, 40000), rs.randint(1, 300, 40000)).astype(np.int32)
    runs[100000:900000] = 0
    assert np.array_equal(_device_hist(gpu, runs, 30000), H.histogram(runs, 30000))


def test_out_of_range_counts_are_skipped_and_nothing_is_written_outside_the_table(gpu):
    rs = np.random.RandomState(23)
    mrd = 777
    counts = rs.randint(-2000, 3000, 1 << 21).astype(np.int32)
    counts[:6] = [-(2 ** 31), 2 ** 31 - 1, mrd, -1, mrd - 1, 0]
    got = _device_hist(gpu, counts, mrd, offset=1)   # (_device_hist checks the guard words)
    in_range = (counts >= 0) & (counts < mrd)
    assert np.array_equal(got, H.histogram(counts, mrd)) and int(got.sum()) == int(in_range.sum()) < counts.size
    # every count out of range: the table stays empty
    assert _device_hist(gpu, np.full(100000, mrd, np.int32), mrd).sum() == 0


PLAIN = {   # name: (view, mrd)
    "cfg2": (View(-2.0, -1.5, 3.0, 3.0, 4096, 4096), 1000),
    "cfg3-like": (View(-0.743648, 0.131820, 1e-5, 1e-5, 1021, 1019), 10000),
    "outside": (View(2.5, 2.5, 1.0, 1.0, 1027, 515), 500),
    "inside": (View(-0.2, -0.1, 0.2, 0.2, 1027, 515), 2000),
}


def _check_against_counts(hist, counts, st, mrd):
    assert hist.dtype == np.uint64 and hist.shape == (mrd,)
    assert np.array_equal(hist, H.histogram(counts, mrd))
    assert int(hist.sum()) == counts.size
    assert int(hist[0]) == st.never_pixels
    first_moment = sum(int(c) * int(h) for c, h in zip(np.nonzero(hist)[0], hist[np.nonzero(hist)[0]]))
    assert first_moment + (mrd - 1) * int(hist[0]) == st.pixel_iterations


@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_view_histograms(gpu, name):
    view, mrd = PLAIN[name]
    counts, _, st = gpu.compute_view(view, mrd, want_bytes=False)
    hist, hst = gpu.view_histogram(view, mrd, want_stats=True)
    _check_against_counts(hist, counts, st, mrd)
    assert (hst.never_pixels, hst.pixel_iterations) == (st.never_pixels, st.pixel_iterations)
    assert hst.kernel_ms > 0 and not hst.all_bytes_zero and not hst.all_bytes_one and hst.rle_runs == 0
    if name == "outside":
        assert hist[1] == counts.size
    if name == "inside":
        assert hist[0] == counts.size
    # the whole view is the sum of its row bands
    total = np.zeros(mrd, np.uint64)
    for r0 in range(0, view.height, 300):
        nr = min(300, view.height - r0)
        band = gpu.view_histogram(view, mrd, window=(0, r0, view.width, nr))
        assert np.array_equal(band, H.histogram(counts[r0:r0 + nr], mrd))
        total += band
    assert np.array_equal(total, hist)
    window = (13, 7, 500, 401)
    assert np.array_equal(gpu.view_histogram(view, mrd, window=window), H.histogram(counts[7:408, 13:513], mrd))
    # every accepted kernel selector gives the same table; fp32 gives the table of the fp32 counts
    if name != "cfg2":
        for kernel in ("simple", "asm", "refill", "group", "scan"):
            assert np.array_equal(gpu.view_histogram(view, mrd, kernel=kernel), hist), kernel
    for kernel in ("default", "asm", "group", "scan"):
        c32, _, _ = gpu.compute_view(view, mrd, want_bytes=False, kernel=kernel, precision="f32")
        assert np.array_equal(gpu.view_histogram(view, mrd, kernel=kernel, precision="f32"), H.histogram(c32, mrd)), kernel


def test_deep_view_histogram(gpu):
    span, mrd = 1e-20, 30000
    orbit = DeepOrbit(*SEAHORSE, mrd, min_span=span)
    view = DeepView(span, 509, 383)
    counts, _, _, st = gpu.compute_deep_view(orbit, view, mrd, want_bytes=False)
    assert len(np.unique(counts)) > 10
    hist, hst = gpu.deep_view_histogram(orbit, view, mrd, want_stats=True)
    _check_against_counts(hist, counts, st, mrd)
    assert (hst.never_pixels, hst.pixel_iterations) == (st.never_pixels, st.pixel_iterations)
    total = np.zeros(mrd, np.uint64)
    for r0 in range(0, view.height, 100):
        total += gpu.deep_view_histogram(orbit, view, mrd, window=(0, r0, view.width, min(100, view.height - r0)))
    assert np.array_equal(total, hist)
    assert np.array_equal(gpu.deep_view_histogram(orbit, view, mrd, window=(5, 9, 300, 200)), H.histogram(counts[9:209, 5:305], mrd))


def test_a_view_of_two_scratch_bands_equals_the_sum_of_its_one_band_windows(gpu):
    w, h, mrd = 8200, 8200, 64
    assert w * h * 4 > L.MBK_RENDER_BAND_BYTES > w * (h // 2) * 4
    view = View(-2.0, -1.25, 2.5, 2.5, w, h)
    hist, st = gpu.view_histogram(view, mrd, want_stats=True)
    parts = [gpu.view_histogram(view, mrd, window=(0, r0, w, h // 2), want_stats=True) for r0 in (0, h // 2)]
    assert np.array_equal(hist, parts[0][0] + parts[1][0]) and int(hist.sum()) == w * h
    assert st.never_pixels == parts[0][1].never_pixels + parts[1][1].never_pixels == int(hist[0])
    assert st.pixel_iterations == parts[0][1].pixel_iterations + parts[1][1].pixel_iterations
    counts, _, _ = gpu.compute_view(view, mrd, window=(0, 0, w, h // 2), want_bytes=False)
    assert np.array_equal(parts[0][0], H.histogram(counts, mrd))


def test_launch_forms_accumulate_into_a_device_table(gpu):
    torch = _torch()
    view, mrd = View(-2.0, -1.5, 3.0, 3.0, 640, 480), 300
    orbit = DeepOrbit("0", "1", 5000, min_span=1e-60)
    dview = DeepView(1e-60, 150, 131)
    stream = torch.cuda.Stream()
    for deep in (False, True):
        m = 5000 if deep else mrd
        want = gpu.deep_view_histogram(orbit, dview, m) if deep else gpu.view_histogram(view, mrd)
        buf = torch.from_numpy(np.full(m + 32, GUARD, np.uint64).view(np.int64)).to("cuda:0")
        buf[16:16 + m] = 0
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for window in ((0, 0, 150, 60), (0, 60, 150, 71)) if deep else ((0, 0, 640, 100), (0, 100, 640, 380)):
                if deep:
                    gpu.launch_deep_view_histogram(orbit, dview, m, d_hist=buf.data_ptr() + 128, stream=stream.cuda_stream, window=window)
                else:
                    gpu.launch_view_histogram(view, mrd, d_hist=buf.data_ptr() + 128, stream=stream.cuda_stream, window=window)
        stream.synchronize()
        got = buf.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[16:16 + m], want), deep
        assert (got[:16] == GUARD).all() and (got[16 + m:] == GUARD).all(), deep


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


def _model(pal, table, s, counts, nu):
    out = [H.render_equalized(pal.entries, pal.inside, pal.scale, pal.offset, table, s, counts[r:r + 64 * s], nu[r:r + 64 * s])
           for r in range(0, counts.shape[0], 64 * s)]
    return np.concatenate(out)


@pytest.mark.parametrize("s", [1, 2])
def test_plain_equalized_render_equals_the_model(gpu, s):
    w, h, mrd = 509, 383, 1500
    view = View(-0.743643 - 5e-6, 0.131825 - 5e-6 * h / w, 1e-5, 1e-5 * h / w, w, h)
    nu, counts, st_s = gpu.compute_view_smooth(_finer(view, s), mrd)
    assert len(np.unique(counts)) > 10
    hist = gpu.view_histogram(view, mrd)                      # the table is that of the view at OUTPUT resolution
    table = equalize_lut(hist)
    assert np.array_equal(table.view(np.uint64), H.lut(hist).view(np.uint64))
    img, st = gpu.render_view(view, mrd, palette=EQ_PAL, source="equalized", supersample=s)
    want = _model(EQ_PAL, table, s, counts, nu)
    assert img.shape == (h, w, 4) and np.array_equal(img, want), int((img != want).any(axis=2).sum())
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > 100
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    # a windowed render is the same rows of the whole image (one table: the whole view's), whatever the band height
    for window in [(0, 40, w, 33), (13, 0, 101, h), (3, 5, 258, 70)]:
        c0, r0, nc, nr = window
        part, _ = gpu.render_view(view, mrd, palette=EQ_PAL, source="equalized", supersample=s, window=window, max_band_rows=16)
        assert np.array_equal(part, img[r0:r0 + nr, c0:c0 + nc]), window
    # a caller's table is honoured
    other = np.sqrt(table)
    img2, _ = gpu.render_view(view, mrd, palette=EQ_PAL, source="equalized", supersample=s, lut=other)
    assert np.array_equal(img2, _model(EQ_PAL, other, s, counts, nu)) and not np.array_equal(img2, img)
    for kernel in ("asm", "group", "scan"):
        again, _ = gpu.render_view(view, mrd, palette=EQ_PAL, source="equalized", supersample=s, kernel=kernel, lut=table)
        assert np.array_equal(again, img), kernel
    # the launch form into a device buffer
    torch = _torch()
    buf = torch.full((4096 + img.size + 4096,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_view(view, mrd, palette=EQ_PAL, d_rgba=buf.data_ptr() + 4096, source="equalized", supersample=s, lut=table,
                           max_band_rows=50)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[4096:4096 + img.size].reshape(img.shape), img)
    assert (got[:4096] == 0xA5).all() and (got[4096 + img.size:] == 0xA5).all()


@pytest.mark.parametrize("s", [1, 2])
def test_deep_equalized_render_equals_the_model(gpu, s):
    span, mrd, w, h = 1e-60, 5000, 253, 189
    orbit = DeepOrbit("0", "1", mrd, min_span=span)
    view = DeepView(span, w, h)
    counts, _, nu, st_s = gpu.compute_deep_view(orbit, DeepView(span, w * s, h * s, view.span_i), mrd, want_bytes=False, want_smooth=True)
    assert len(np.unique(counts)) > 10
    table = equalize_lut(gpu.deep_view_histogram(orbit, view, mrd))
    img, st = gpu.render_deep_view(orbit, view, mrd, palette=EQ_PAL, source="equalized", supersample=s)
    want = _model(EQ_PAL, table, s, counts, nu)
    assert np.array_equal(img, want), int((img != want).any(axis=2).sum())
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    c0, r0, nc, nr = 17, 9, 150, 77
    part, _ = gpu.render_deep_view(orbit, view, mrd, palette=EQ_PAL, source="equalized", supersample=s, window=(c0, r0, nc, nr))
    assert np.array_equal(part, img[r0:r0 + nr, c0:c0 + nc])
    other = table * table
    img2, _ = gpu.render_deep_view(orbit, view, mrd, palette=EQ_PAL, source="equalized", supersample=s, lut=other)
    assert np.array_equal(img2, _model(EQ_PAL, other, s, counts, nu))
    torch = _torch()
    buf = torch.full((img.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_deep_view(orbit, view, mrd, palette=EQ_PAL, d_rgba=buf.data_ptr(), source="equalized", supersample=s, lut=table)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:img.size].reshape(img.shape), img) and (got[img.size:] == 0xA5).all()


def test_refusals_leave_the_outputs_untouched(gpu):
    torch = _torch()
    lib = L.load()
    view = View(-2.0, -1.5, 3.0, 3.0, 64, 48)
    mrd = 256
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    cv = gpu._cview(view, None)
    dv = gpu._cdeep(DeepView(1e-20, 64, 48), None)
    bad = L.MBK_ERR_INVALID

    # -- histograms: host table of the synchronous forms, device table of the launch forms
    hist = np.full(mrd, GUARD, np.uint64)

    def plain(v=cv, m=mrd, flags=0, dst=hist):
        st = lib.mbk_view_histogram_compute(gpu._h, C.byref(v) if v is not None else None, m, flags,
                                            dst.ctypes.data if dst is not None else None, None)
        assert (hist == GUARD).all()
        return st

    def deep(orb=orbit, v=dv, m=mrd, flags=0, dst=hist):
        st = lib.mbk_deep_view_histogram_compute(gpu._h, orb._h if orb is not None else None, C.byref(v), m, flags,
                                                 dst.ctypes.data if dst is not None else None, None)
        assert (hist == GUARD).all()
        return st

    cases = {
        "NULL view": lambda: plain(v=None), "NULL table": lambda: plain(dst=None), "mrd 0": lambda: plain(m=0),
        "mrd above the limit": lambda: plain(m=L.MBK_HISTOGRAM_MAX_MRD + 1, dst=hist),
        "window exceeds the view": lambda: plain(v=gpu._cview(view, (1, 0, 64, 48))), "empty window": lambda: plain(v=gpu._cview(view, (0, 0, 0, 48))),
        "view not finite": lambda: plain(v=gpu._cview(View(np.nan, -1.5, 3.0, 3.0, 64, 48), None)),
        "unknown kernel": lambda: plain(flags=0x700), "an output flag": lambda: plain(flags=L.MBK_WANT_COUNTS),
        "lazy uniform": lambda: plain(flags=L.MBK_LAZY_UNIFORM), "fp32 with simple": lambda: plain(flags=L.MBK_PRECISION_F32 | L.MBK_KERNEL_SIMPLE),
        "fp32 with refill": lambda: plain(flags=L.MBK_PRECISION_F32 | L.MBK_KERNEL_REFILL),
        "deep: NULL orbit": lambda: deep(orb=None), "deep: NULL table": lambda: deep(dst=None), "deep: mrd 0": lambda: deep(m=0),
        "deep: beyond the orbit's mrd": lambda: deep(m=501), "deep: a flag": lambda: deep(flags=L.MBK_KERNEL_GROUP),
        "deep: fp32": lambda: deep(flags=L.MBK_PRECISION_F32), "deep: range": lambda: deep(v=gpu._cdeep(DeepView(8.0, 64, 48, 8.0), None)),
        "deep: mrd above the limit": lambda: deep(m=L.MBK_HISTOGRAM_MAX_MRD + 1),
    }
    for name, call in cases.items():
        assert call() == bad, name

    d_hist = torch.from_numpy(np.full(mrd + 2, GUARD, np.uint64).view(np.int64)).to("cuda:0")
    d_counts = torch.zeros(1024, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p_hist, p_counts = d_hist.data_ptr() + 8, d_counts.data_ptr()
    assert lib.mbk_counts_histogram(gpu._h, None, 1024, mrd, p_hist, None) == bad
    assert lib.mbk_counts_histogram(gpu._h, p_counts, 1024, mrd, None, None) == bad
    assert lib.mbk_counts_histogram(gpu._h, p_counts, 1024, 0, p_hist, None) == bad
    assert lib.mbk_counts_histogram(gpu._h, p_counts, 1024, L.MBK_HISTOGRAM_MAX_MRD + 1, p_hist, None) == bad
    assert lib.mbk_counts_histogram(gpu._h, p_counts + 2, 1000, mrd, p_hist, None) == bad      # misaligned counts
    assert lib.mbk_counts_histogram(gpu._h, p_counts, 1024, mrd, p_hist + 4, None) == bad      # misaligned table
    assert lib.mbk_counts_histogram(None, p_counts, 1024, mrd, p_hist, None) == bad
    assert lib.mbk_view_histogram_launch(gpu._h, C.byref(cv), 0, 0, p_hist, None) == bad
    assert lib.mbk_view_histogram_launch(gpu._h, C.byref(cv), mrd, 0, None, None) == bad
    assert lib.mbk_view_histogram_launch(gpu._h, C.byref(cv), mrd, 0x700, p_hist, None) == bad
    assert lib.mbk_view_histogram_launch(gpu._h, C.byref(cv), mrd, 0, p_hist + 4, None) == bad
    assert lib.mbk_deep_view_histogram_launch(gpu._h, None, C.byref(dv), mrd, 0, p_hist, None) == bad
    assert lib.mbk_deep_view_histogram_launch(gpu._h, orbit._h, C.byref(dv), 501, 0, p_hist, None) == bad
    assert lib.mbk_deep_view_histogram_launch(gpu._h, orbit._h, C.byref(dv), mrd, L.MBK_KERNEL_ASM, p_hist, None) == bad
    assert lib.mbk_counts_histogram(gpu._h, p_counts, 0, mrd, p_hist, None) == L.MBK_OK         # nothing to add
    torch.cuda.synchronize()
    assert (d_hist.cpu().numpy().view(np.uint64) == GUARD).all()

    # -- equalized renders
    pal = np.zeros((4, 4), np.uint8)
    table = np.linspace(0.0, 1.0, mrd + 2)
    out = np.full((48, 64, 4), 0xA5, np.uint8)

    def spec(source=L.MBK_RENDER_EQUALIZED, s=1, n=4, scale=3.0, offset=0.0, palette=pal):
        return L.mbk_render_spec(source, s, palette.ctypes.data if palette is not None else None, n, (C.c_uint8 * 4)(0, 0, 0, 255),
                                 scale, offset, 0)

    def eq(sp, lut=table, lut_len=None, m=mrd, flags=0, dst=out, v=cv):
        st = lib.mbk_view_render_equalized_compute(gpu._h, C.byref(v), m, flags, C.byref(sp) if sp is not None else None,
                                                   lut.ctypes.data if lut is not None else None,
                                                   (lut.size if lut is not None else 0) if lut_len is None else lut_len,
                                                   dst.ctypes.data if dst is not None else None, None)
        assert (out == 0xA5).all()
        return st

    def deq(sp, lut=table, lut_len=None, m=mrd, flags=0, orb=orbit):
        st = lib.mbk_deep_view_render_equalized_compute(gpu._h, orb._h if orb is not None else None, C.byref(dv), m, flags, C.byref(sp),
                                                        lut.ctypes.data if lut is not None else None,
                                                        (lut.size if lut is not None else 0) if lut_len is None else lut_len,
                                                        out.ctypes.data, None)
        assert (out == 0xA5).all()
        return st

    def entry(k, x):
        t = table.copy()
        t[k] = x
        return t

    pal256 = np.zeros((256, 4), np.uint8)
    cases = {
        "NULL spec": lambda: eq(None), "NULL palette": lambda: eq(spec(palette=None)), "NULL output": lambda: eq(spec(), dst=None),
        "NULL table": lambda: eq(spec(), lut=None, lut_len=mrd + 2), "lut_len mrd + 1": lambda: eq(spec(), lut_len=mrd + 1),
        "lut_len mrd + 3": lambda: eq(spec(), lut=np.zeros(mrd + 3), lut_len=mrd + 3), "lut_len 0": lambda: eq(spec(), lut_len=0),
        "entry > 1": lambda: eq(spec(), lut=entry(5, 1.5)), "entry < 0": lambda: eq(spec(), lut=entry(0, -0.25)),
        "entry nan": lambda: eq(spec(), lut=entry(mrd + 1, np.nan)), "entry inf": lambda: eq(spec(), lut=entry(9, np.inf)),
        "source smooth": lambda: eq(spec(source=L.MBK_RENDER_SMOOTH)), "source bytes": lambda: eq(spec(source=L.MBK_RENDER_BYTES, n=256, palette=pal256)),
        "source distance": lambda: eq(spec(source=L.MBK_RENDER_DISTANCE)), "source 2": lambda: eq(spec(source=2)),
        "palette of 1": lambda: eq(spec(n=1)), "s = 5": lambda: eq(spec(s=5)), "scale 0": lambda: eq(spec(scale=0.0)),
        "scale > 2^20": lambda: eq(spec(scale=2.0 ** 21)), "offset nan": lambda: eq(spec(offset=np.nan)),
        "mrd above the limit": lambda: eq(spec(), m=L.MBK_HISTOGRAM_MAX_MRD + 1, lut=np.zeros(L.MBK_HISTOGRAM_MAX_MRD + 3)),
        "simple": lambda: eq(spec(), flags=L.MBK_KERNEL_SIMPLE), "refill": lambda: eq(spec(), flags=L.MBK_KERNEL_REFILL),
        "fp32": lambda: eq(spec(), flags=L.MBK_PRECISION_F32), "an output flag": lambda: eq(spec(), flags=L.MBK_WANT_COUNTS),
        "window exceeds the view": lambda: eq(spec(), v=gpu._cview(view, (1, 0, 64, 48))),
        "deep: NULL orbit": lambda: deq(spec(), orb=None), "deep: beyond the orbit's mrd": lambda: deq(spec(), m=501, lut=np.zeros(503)),
        "deep: a flag": lambda: deq(spec(), flags=L.MBK_KERNEL_GROUP), "deep: lut_len": lambda: deq(spec(), lut_len=mrd + 1),
        "deep: entry": lambda: deq(spec(), lut=entry(3, 2.0)), "deep: source smooth": lambda: deq(spec(source=L.MBK_RENDER_SMOOTH)),
        "deep: source distance_rel": lambda: deq(spec(source=L.MBK_RENDER_DISTANCE_REL)),
    }
    for name, call in cases.items():
        assert call() == bad, name
    # the calls without a table refuse the source
    assert lib.mbk_view_render_compute(gpu._h, C.byref(cv), mrd, 0, C.byref(spec()), out.ctypes.data, None) == bad
    assert lib.mbk_deep_view_render_compute(gpu._h, orbit._h, C.byref(dv), mrd, 0, C.byref(spec()), out.ctypes.data, None) == bad
    assert (out == 0xA5).all()
    with pytest.raises(MbkError):
        gpu.render_view(view, mrd, palette=EQ_PAL, source="equalized", lut=table[:-1])
    # the launch forms refuse the same way: a device buffer stays as it was
    buf = torch.full((48 * 64 * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for sp, lut in ((spec(source=L.MBK_RENDER_SMOOTH), table), (spec(), entry(1, -1.0)), (spec(s=5), table)):
        assert lib.mbk_view_render_equalized_launch(gpu._h, C.byref(cv), mrd, 0, C.byref(sp), lut.ctypes.data, lut.size,
                                                    buf.data_ptr(), None) == bad
        assert lib.mbk_deep_view_render_equalized_launch(gpu._h, orbit._h, C.byref(dv), mrd, 0, C.byref(sp), lut.ctypes.data, lut.size,
                                                         buf.data_ptr(), None) == bad
    assert lib.mbk_view_render_equalized_launch(gpu._h, C.byref(cv), mrd, 0, C.byref(spec()), table.ctypes.data, table.size - 1,
                                                buf.data_ptr(), None) == bad
    assert lib.mbk_view_render_launch(gpu._h, C.byref(cv), mrd, 0, C.byref(spec()), buf.data_ptr(), None) == bad
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all()
    # slot 0 busy: the synchronous forms are refused, and work again after the wait
    tile = gpu.pinned_empty((L.MBK_CHUNK_BYTES,), np.uint8)
    gpu.submit_datachunk(0, 4, 256, 1, 2, tile)
    assert plain() == bad and deep() == bad and eq(spec()) == bad
    gpu.wait(0)
    ok = np.empty((48, 64, 4), np.uint8)
    assert lib.mbk_view_render_equalized_compute(gpu._h, C.byref(cv), mrd, 0, C.byref(spec()), table.ctypes.data, table.size,
                                                 ok.ctypes.data, None) == L.MBK_OK
    h2 = np.empty(mrd, np.uint64)
    assert lib.mbk_view_histogram_compute(gpu._h, C.byref(cv), mrd, 0, h2.ctypes.data, None) == L.MBK_OK and h2.sum() == 64 * 48
