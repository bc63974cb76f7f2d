"""Distance estimates for Julia views on the GPU (include/mbk.h, the section of that name), held to the numpy model of the
contract (tests/julia_distance_model.py) and to the truth of the output expression.

The counts are compared with compute_julia_view's bit for bit.  The states behind de (z, d, mag, dmag) are exact in the
model, so the device's de must be the model's value wherever ocml's ln and numpy's agree, and elsewhere the value a
neighbouring ln gives (assert_states_agree), and every sample is within J_GPU = J0 + 1 ulp(de) of the correctly rounded
expression at the model's (mag, dmag).  Both designs run everywhere: kernel "asm" is the one-pass form, "default" and "group"
the two-pass form.

Measured on gfx950 (ocml, ROCm 7): every sample of every small case equals the numpy model bit for bit, with every kernel, cycle
test on and off, except 0.02 % of c = i and 0.05 % of c = -0.8 + 1e-301i, which are a neighbouring ln's value; worst 2.002
ulp(de) against the correctly rounded expression (n = 1, mag = 37149473443.602585, dmag = 8582448776673.926; allowed 3.01), to
the digits of glibc.  c = -2 lines: de / t in [3.99999997, 4.00333000] left of the tip, [2.00000000, 2.00001956] above 0.5, the
CPU model's figures.
"""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import julia_distance_model as JM
from distributedmandelbrot_amd import MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _error_text
from distributedmandelbrot_amd.image import resolve_host

pytestmark = pytest.mark.gpu

KERNELS = ["default", "asm", "group"]
_HELD = set()       # (case, sha256 of de): arrays already held to the truth of the expression


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
    """Seven parameters on a ragged view (fused and literal doubling, |c|^2 = 4, |c| > 2), the critical point, ragged
    windows, a 1 x 1 view and coordinates at 2^499."""
    dev = gpu if cycle else strict
    assert dev.get_option("cycle_detect") == cycle
    for case in JM.SMALL_CASES:
        name, v, c, mrd, window = case
        what = f"{name} {kernel} cycle={cycle}"
        mde, mn, st = JM.case_model(case)
        counts, _, _, _ = dev.compute_julia_view(View(*v), c, mrd, window=window, want_bytes=False, kernel=kernel)
        de, n, stats = dev.compute_julia_view_distance(View(*v), c, mrd, window=window, kernel=kernel)
        assert de.shape == n.shape == mn.shape and de.dtype == np.float64 and n.dtype == np.int32
        assert np.array_equal(n, counts), (what, int((n != counts).sum()))
        assert np.array_equal(n, mn), (what, int((n != mn).sum()))
        assert not np.isnan(de).any() and np.array_equal(de == 0.0, n == 0) and (de >= 0.0).all(), what
        share = JM.assert_states_agree(de, st, what)
        print(f"{what}: {100 * share:.2f} % of the samples equal the numpy model bit for bit")
        key = (name, hashlib.sha256(de.tobytes()).hexdigest())
        if key not in _HELD:        # (the same bytes need no second look)
            JM.assert_expression_within(de, st, what, JM.J_GPU)
            _HELD.add(key)
        assert stats.pixel_iterations == int(np.where(n > 0, n, max(mrd - 1, 0)).astype(np.int64).sum()), what
        assert stats.never_pixels == int((n == 0).sum()), what
        if name == "critical":      # z_0 = 0 at the centre: d = 0 from the first step on
            assert n[32, 32] == 19 and np.flatnonzero(np.isinf(de)).tolist() == [32 * 65 + 32]
        if name == "2^499":
            assert (de == math.inf).all()
        if name == "neck":
            assert int((n == 0).sum()) == 1067


BIG = (View(-1.6, -1.6, 3.2, 3.2, 2048, 2048), (-0.8, 0.156), 500)
# (the windows of BIG_WINDOWS in tests/test_gpu_distance.py)
BIG_WINDOWS = [(0, 1000, 2048, 8), (0, 1021, 2048, 3), (0, 2045, 2048, 3), (300, 700, 513, 129), (2047, 2047, 1, 1),
               (13, 0, 1, 2048), (1023, 1023, 2, 2)]
_BIG = {}


def _big(gpu):
    """The whole view with the default kernel, computed once: read-only."""
    if not _BIG:
        view, c, mrd = BIG
        _BIG["de"], _BIG["n"], _ = gpu.compute_julia_view_distance(view, c, mrd)
    return _BIG["de"], _BIG["n"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_window_equals_the_same_pixels_of_the_whole_view(gpu, kernel):
    view, c, mrd = BIG
    ref_de, ref_n = _big(gpu)
    whole, wn, _ = gpu.compute_julia_view_distance(view, c, mrd, kernel=kernel)
    counts, _, _, _ = gpu.compute_julia_view(view, c, mrd, want_bytes=False)
    assert np.array_equal(wn, counts) and len(np.unique(wn)) >= 100
    assert np.array_equal(whole == 0.0, wn == 0) and not np.isnan(whole).any()
    assert np.array_equal(whole, ref_de) and np.array_equal(wn, ref_n)         # the two designs store the same values
    for window in BIG_WINDOWS:
        c0, r0, nc, nr = window
        de, n, st = gpu.compute_julia_view_distance(view, c, mrd, window=window, kernel=kernel)
        assert np.array_equal(n, wn[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(de, whole[r0:r0 + nr, c0:c0 + nc]), window
        assert st.pixel_iterations == int(np.where(n > 0, n, mrd - 1).astype(np.int64).sum()), window


def _device_buffers(torch, px, guard):
    dd = torch.full((px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    return dd, dc


@pytest.mark.parametrize("kernel", KERNELS)
def test_launch_form_on_a_torch_stream(gpu, kernel):
    """Device pointers, the caller's stream, with a counts buffer and with d_counts = 0 (the scratch counts): the same de
    bits as compute_julia_view_distance, and the guard elements either side of the window-sized buffers keep their
    sentinels."""
    import torch
    view, c, mrd = View(-1.6, -1.2, 3.2, 2.4, 301, 203), (-0.75, 0.0) if kernel == "asm" else (-0.8, 0.156), 400
    guard = 1024
    stream = torch.cuda.Stream(device="cuda:0")
    whole_de, whole_n, _ = gpu.compute_julia_view_distance(view, c, mrd, kernel=kernel)
    assert (whole_n > 0).any()
    for window in (None, (37, 101, 133, 77), (0, 100, 301, 8), (300, 202, 1, 1)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        want_de, want_n = whole_de[r0:r0 + nr, c0:c0 + nc], whole_n[r0:r0 + nr, c0:c0 + nc]
        px = want_de.size
        bufs = [_device_buffers(torch, px, guard) for _ in range(2)]
        torch.cuda.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            gpu.launch_julia_view_distance(view, c, mrd, d_distance=dd[guard:].data_ptr(),
                                           d_counts=dc[guard:].data_ptr() if with_counts else 0, stream=stream.cuda_stream,
                                           window=window, kernel=kernel)
        stream.synchronize()
        for (dd, dc), with_counts in zip(bufs, (True, False)):
            hd, hc = dd.cpu().numpy(), dc.cpu().numpy()
            assert np.array_equal(hd[guard:guard + px].reshape(want_de.shape).view(np.uint64), want_de.view(np.uint64)), (window, with_counts)
            assert (hd[:guard] == -77.0).all() and (hd[guard + px:] == -77.0).all(), (window, with_counts)
            assert (hc[:guard] == -5).all() and (hc[guard + px:] == -5).all(), (window, with_counts)
            if with_counts:
                assert np.array_equal(hc[guard:guard + px].reshape(want_n.shape), want_n), window
            else:
                assert (hc == -5).all(), window


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


@pytest.mark.parametrize("kernel", ["default", "asm"])
@pytest.mark.parametrize("s", [1, 2])
def test_render_equals_the_host_rule_on_the_devices_own_samples(gpu, s, kernel):
    """render_julia_view_distance is mbk_render_resolve_host with source "distance" (held to the numpy rule by
    tests/test_distance.py) of the samples compute_julia_view_distance returns for the s times finer view; banded and
    unbanded, whole and windowed, and the launch form.  The never-escaped samples take `inside`."""
    w, h = 253, 189
    view, c, mrd = View(-1.6, -1.2, 3.2, 2.4, w, h), (-0.75, 0.0), 300
    inside = (9, 8, 7, 255)
    pal = Palette(np.random.RandomState(7).randint(0, 256, (300, 4)).astype(np.uint8), inside=inside).for_distance(view, 12.0)
    de, counts, st_s = gpu.compute_julia_view_distance(_finer(view, s), c, mrd, kernel=kernel)
    assert len(np.unique(counts)) > 10 and (counts == 0).any()
    want = resolve_host(pal, "distance", s, w, h, counts=counts, smooth=de)
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    for rows in (0, 8):
        img, st = gpu.render_julia_view_distance(view, c, mrd, palette=pal, supersample=s, kernel=kernel, max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    if s == 1:
        assert (img[counts == 0] == np.array(inside, np.uint8)).all()
    else:       # an output pixel whose four samples all stay inside
        allin = (counts.reshape(h, s, w, s) == 0).all(axis=(1, 3))
        assert allin.any() and (img[allin] == np.array(inside, np.uint8)).all()
    window = (100, 50, 77, 53)
    img, _ = gpu.render_julia_view_distance(view, c, mrd, palette=pal, supersample=s, kernel=kernel, window=window)
    assert np.array_equal(img, want[50:103, 100:177])
    import torch
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    gpu.launch_render_julia_view_distance(view, c, mrd, palette=pal, d_rgba=d.data_ptr(), supersample=s, kernel=kernel)
    torch.cuda.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


KERNEL_TEXT = "Julia views are implemented by MBK_KERNEL_DEFAULT / _ASM / _GROUP only"
FLAG_TEXT = "Julia distance estimates take kernel selection only"


def test_refusals_by_message_and_nothing_written(gpu):
    import torch
    lib = gpu._lib
    bad = L.MBK_ERR_INVALID
    view = View(-1.6, -1.2, 3.2, 2.4, 16, 16)
    cv = gpu._cview(view, None)
    c, mrd, px, guard = (-0.8, 0.156), 100, 256, 64
    dd, dc = _device_buffers(torch, px, guard)
    d_rgba = torch.full((px + 2 * guard,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pd, pc, pr = dd[guard:].data_ptr(), dc[guard:].data_ptr(), d_rgba[guard:].data_ptr()
    h_de, h_n, h_rgba = np.full(px, -1.0), np.full(px, -9, np.int32), np.full(px * 4, 0xA5, np.uint8)
    pal = Palette.distance(view, 8.0, inner_px=1.0)

    def refused(rc, text, what):
        assert rc == bad, what
        assert text in _error_text(lib, gpu._h), (what, _error_text(lib, gpu._h))

    def values(flags=0, c=c, mrd=mrd, v=cv, de=True):
        """(status of the launch form, status of the compute form)"""
        vp = C.byref(v) if v is not None else None
        return (lib.mbk_julia_view_launch_distance(gpu._h, vp, c[0], c[1], mrd, flags, pc, pd if de else None, None),
                lib.mbk_julia_view_compute_distance(gpu._h, vp, c[0], c[1], mrd, flags, h_n.ctypes.data,
                                                    h_de.ctypes.data if de else None, None))

    def renders(flags=0, c=c, mrd=mrd, v=cv, source="distance", out=True, p=pal):
        vp = C.byref(v) if v is not None else None
        spec = p.spec(source, 1)
        return (lib.mbk_julia_view_distance_render_launch(gpu._h, vp, c[0], c[1], mrd, flags, C.byref(spec), pr if out else None, None),
                lib.mbk_julia_view_distance_render_compute(gpu._h, vp, c[0], c[1], mrd, flags, C.byref(spec),
                                                           h_rgba.ctypes.data if out else None, None))

    cases = {
        "simple": (dict(flags=L.MBK_KERNEL_SIMPLE), KERNEL_TEXT), "refill": (dict(flags=L.MBK_KERNEL_REFILL), KERNEL_TEXT),
        "scan": (dict(flags=L.MBK_KERNEL_SCAN), KERNEL_TEXT), "selector 0x600": (dict(flags=0x600), KERNEL_TEXT),
        "fp32": (dict(flags=L.MBK_PRECISION_F32), FLAG_TEXT), "lazy": (dict(flags=L.MBK_LAZY_UNIFORM), FLAG_TEXT),
        "bla": (dict(flags=L.MBK_DEEP_BLA), FLAG_TEXT), "xbla": (dict(flags=L.MBK_DEEP_XBLA), FLAG_TEXT),
        "want counts": (dict(flags=L.MBK_WANT_COUNTS), FLAG_TEXT), "bit 30": (dict(flags=1 << 30), FLAG_TEXT),
        "asm + fp32": (dict(flags=L.MBK_KERNEL_ASM | L.MBK_PRECISION_F32), FLAG_TEXT),
        "c inf": (dict(c=(math.inf, 0.0)), "the Julia parameter must be finite"),
        "c nan": (dict(c=(0.0, math.nan)), "the Julia parameter must be finite"),
        "mrd 2^31": (dict(mrd=1 << 31), "mrd must fit int32"),
        "window exceeds the view": (dict(v=gpu._cview(view, (10, 0, 7, 16))), ""),
        "coordinates beyond 2^500": (dict(v=gpu._cview(View(2.0 ** 500, 0.0, 2.0 ** 500, 1.0, 4, 4), None)), ""),
        "NULL view": (dict(v=None), ""),
    }
    for name, (kw, text) in cases.items():
        for rc in values(**kw) + renders(**kw):
            refused(rc, text, name)
    for rc in values(de=False):
        refused(rc, "NULL value pointer", "NULL distance")
    for rc in renders(out=False):
        refused(rc, "output pointer is NULL", "NULL rgba")
    for source in ("bytes", "smooth", "distance_rel"):
        p = Palette(np.zeros((256, 4), np.uint8), scale=1.0)
        for rc in renders(source=source, p=p):
            refused(rc, "Julia distance renders take MBK_RENDER_DISTANCE only", source)
    for rc in renders(source="equalized", p=Palette(np.zeros((256, 4), np.uint8), scale=1.0)):
        assert rc == bad
    for p in (Palette(pal.entries, scale=2.0 ** 81), Palette(pal.entries, scale=0.0), Palette(pal.entries[:1])):
        for rc in renders(p=p):
            assert rc == bad
    # the Python layer raises them
    with pytest.raises(MbkError, match="DEFAULT / _ASM / _GROUP"):
        gpu.compute_julia_view_distance(view, c, mrd, kernel="scan")
    with pytest.raises(MbkError, match="NULL value pointer"):
        gpu.launch_julia_view_distance(view, c, mrd, d_distance=0, d_counts=pc)
    with pytest.raises(MbkError, match="DEFAULT / _ASM / _GROUP"):
        gpu.render_julia_view_distance(view, c, mrd, palette=pal, kernel="simple")
    # mbk_julia_view_render_* keeps refusing the distance sources, message unchanged
    with pytest.raises(MbkError, match=r"implemented for Mandelbrot views only \(no Julia renders\)"):
        gpu.render_julia_view(view, c, mrd, palette=pal, source="distance")
    torch.cuda.synchronize()
    assert (dd.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all() and (d_rgba.cpu().numpy() == -3).all()
    assert (h_de == -1.0).all() and (h_n == -9).all() and (h_rgba == 0xA5).all()
    # and the calls work: NULL counts in both forms, trivial depths
    assert lib.mbk_julia_view_compute_distance(gpu._h, C.byref(cv), c[0], c[1], mrd, 0, None, h_de.ctypes.data, None) == L.MBK_OK
    want, _, _ = gpu.compute_julia_view_distance(view, c, mrd)
    assert np.array_equal(h_de.reshape(16, 16), want) and (h_n == -9).all()
    for m in (0, 1):
        for kernel in KERNELS:
            de, n, st = gpu.compute_julia_view_distance(view, c, m, kernel=kernel)
            assert not de.any() and not n.any() and st.pixel_iterations == 0 and st.never_pixels == 256


TS = np.logspace(-2, -12, 41)


def _gpu_line(gpu, zr0, zi0, c, mrd, kernel):
    """The samples (zr0[k], zi0[k]) as 1 x 1 views (a view is a linspace; the lines are log-spaced)."""
    de = np.empty(zr0.size)
    for k in range(zr0.size):
        d, n, _ = gpu.compute_julia_view_distance(View(float(zr0[k]), float(zi0[k]), 0.0, 0.0, 1, 1), c, mrd, kernel=kernel)
        assert n[0, 0] > 0, (k, "mrd too small")
        de[k] = d[0, 0]
    return de


@pytest.mark.parametrize("kernel", ["default", "asm"])
def test_segment_lines_on_the_device(gpu, kernel):
    """The two c = -2 lines of tests/test_julia_distance.py on the device's own output: Koebe's 4 left of the tip, 2 above
    an inner point of the segment."""
    c, mrd = (-2.0, 0.0), 4000
    for zr0, zi0, lo, hi, what in ((-2.0 - TS, np.zeros_like(TS), 3.99, 4.01, "tip"), (np.full_like(TS, 0.5), TS.copy(), 1.99, 2.01, "above 0.5")):
        dist = np.hypot(zr0 - np.clip(zr0, -2.0, 2.0), zi0)
        ratio = _gpu_line(gpu, zr0, zi0, c, mrd, kernel) / dist
        print(f"c = -2 {what} {kernel}: de / t in [{ratio.min():.8f}, {ratio.max():.8f}]")
        assert (ratio >= lo).all() and (ratio <= hi).all(), (what, float(ratio.min()), float(ratio.max()))
