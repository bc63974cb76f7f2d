"""The continuous escape-time output (BASELINE cfg5) of plain views on the GPU, held to the truth.

nu = n + 1 - log2(0.5 ln mag) is compared with tests/smooth_truth.nu_true (mpmath on the exact binary64 mag that the C
oracle reports for the pixel) on every kernel that implements it, with the cycle test on and off, at the shapes,
windows and magnitudes where the count tests already go, and through mbk_view_launch_smooth, the entry point the
benchmark times.  The bound is err <= A ulp(nu) + B 2^-52 with A = A0 + 1, B = B0 + 2 (smooth_truth.py says why).

Measured (glibc libm on x86-64 / ocml on gfx950, ROCm 7):

    CPU reference   A0 = 1.5698 ulp(nu)   at n = 1, mag = 11337031.25        ("far" view, nu = -1.02)
                    B0 = 1.3786 x 2^-52   at n = 1, mag = 75820.85571289062  ("far" view, nu = -0.49)
    GPU, allowed    A  = 2.57,  B = 3.38
    GPU, measured   A  = 1.570 ulp(nu) and B = 1.379 x 2^-52, at the same two pixels and to the same digits as glibc:
                    ocml and glibc round both logarithms alike there; over cfg5 the two differ by at most 2.8e-14
                    (n ~ 100) and the worst of its 21 996 sampled pixels is 1.195 ulp at n = 1, mag = 18.177277466062407

Whole arrays are compared with the oracle's by the sum of the two bounds.  Counts are compared with the oracle's bit for
bit everywhere; nu is 0 exactly where the count is 0 and -inf exactly where mag overflowed.
"""
import ctypes as C
import hashlib
import json
import math
import os

import numpy as np
import pytest

import smooth_truth as T
from distributedmandelbrot_amd import MbkError, View
from distributedmandelbrot_amd import _lib as L

pytestmark = pytest.mark.gpu

SMOOTH_KERNELS = ["default", "asm", "group", "scan"]
NU_AT_MINUS_2 = 2.5287663729448977          # 2 - log2(ln 2), correctly rounded

_TRUTH = {}


def _small_case(oracle, case):
    """Oracle (nu, counts, mag) and the truth (near, rest) of a T.SMALL_CASES entry, computed once."""
    name, v, mrd, window = case
    if name not in _TRUTH:
        osm, oc, mag = oracle.view_smooth_mag(*v, mrd, window=window)
        _TRUTH[name] = (osm, oc, mag, T.nu_true_array(oc.ravel(), mag.ravel()))
    return _TRUTH[name]


@pytest.fixture(scope="module")
def strict():
    """A second ctx with the cycle test off (every pixel runs the reference loop to its end)."""
    from distributedmandelbrot_amd import MandelbrotDevice
    with MandelbrotDevice(0) as dev:
        dev.set_option("cycle_detect", 0)
        yield dev


@pytest.mark.parametrize("cycle", [1, 0], ids=["cycle", "strict"])
@pytest.mark.parametrize("kernel", SMOOTH_KERNELS)
def test_small_views_every_escaped_pixel(gpu, strict, oracle, kernel, cycle):
    """1-wide, 1-high and ragged views, offset windows, step-zero axes, tiny imaginary parts (the exact-doubling path),
    the |c| = 2 ring, |c| up to 74 (nu passes through 0), and magnitudes up to and past the binary64 overflow: counts
    equal the oracle's, nu is 0 exactly where the count is 0, every escaped pixel is within the bound of the truth, and
    the statistics are those of the window."""
    dev = gpu if cycle else strict
    assert dev.get_option("cycle_detect") == cycle
    for case in T.SMALL_CASES:
        name, v, mrd, window = case
        osm, oc, mag, truth = _small_case(oracle, case)
        sm, c, st = dev.compute_view_smooth(View(*v), mrd, window=window, kernel=kernel)
        what = f"{name} {kernel} cycle={cycle}"
        assert sm.shape == c.shape == oc.shape
        assert np.array_equal(c, oc), (what, int((c != oc).sum()))
        T.assert_within(sm, oc, mag, what, truth=truth)
        T.assert_pair(sm, osm, oc, what)
        assert st.pixel_iterations == int(np.where(oc > 0, oc, mrd - 1).astype(np.int64).sum()), what
        assert st.never_pixels == int((oc == 0).sum()), what
        if name == "ring":          # c = -2 + 0i: z_1 = 2, mag = 4.0 exactly
            assert (c[16, 0], mag[16, 0]) == (1, 4.0)
            assert abs(sm[16, 0] - NU_AT_MINUS_2) <= T.bound(NU_AT_MINUS_2), sm[16, 0]
            top = oc[oc > 0] + (NU_AT_MINUS_2 - 1)                  # mag >= 4: nu <= n + 1 - log2(ln 2)
            assert (sm[oc > 0] <= top + T.bound(top) + T.ulp(top)).all()
        if name == "huge":          # mag crosses the overflow inside the view
            assert (c == 1).all() and np.isinf(sm).any() and np.isfinite(sm).any()
            assert np.array_equal(np.isinf(sm), np.isinf(mag)) and (sm[np.isinf(mag)] == -math.inf).all()
            assert mag[np.isfinite(mag)].max() > 1e305
        if name == "2^499":
            assert (c == 1).all() and (sm == -math.inf).all()


BIG = (View(-2.0, -1.5, 3.0, 3.0, 2048, 2048), 500)
BIG_WINDOWS = [(0, 1000, 2048, 8), (0, 1021, 2048, 3), (0, 2045, 2048, 3), (300, 700, 513, 129), (2047, 2047, 1, 1),
               (13, 0, 1, 2048), (1023, 1023, 2, 2)]


@pytest.mark.parametrize("kernel", SMOOTH_KERNELS)
def test_window_equals_the_same_pixels_of_the_whole_view(gpu, oracle, kernel):
    """The coordinates of a pixel do not depend on the window: a window's nu and counts equal, bit for bit, the same rows
    and columns of the whole view's (the same kernel: equality, not a tolerance).  Full-width 8-row and 3-row bands of a
    2048-wide view are the shard unit.  The statistics are the window's."""
    view, mrd = BIG
    whole, wc, wst = gpu.compute_view_smooth(view, mrd, kernel=kernel)
    assert len(np.unique(wc)) >= 100 and (wc == 0).any()
    assert wst.pixel_iterations == int(np.where(wc > 0, wc, mrd - 1).astype(np.int64).sum())
    for window in BIG_WINDOWS:
        c0, r0, nc, nr = window
        sm, c, st = gpu.compute_view_smooth(view, mrd, window=window, kernel=kernel)
        assert sm.shape == (nr, nc)
        assert np.array_equal(c, wc[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(sm, whole[r0:r0 + nr, c0:c0 + nc]), (window, int((sm != whole[r0:r0 + nr, c0:c0 + nc]).sum()))
        assert st.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum()), window
        assert st.never_pixels == int((c == 0).sum()), window
    # and the band is right, not only consistent: against the truth
    window = BIG_WINDOWS[0]
    osm, oc, mag = oracle.view_smooth_mag(view.start_r, view.start_i, view.range_r, view.range_i, view.width, view.height,
                                          mrd, window=window)
    sm, c, _ = gpu.compute_view_smooth(view, mrd, window=window, kernel=kernel)
    assert np.array_equal(c, oc)
    T.assert_within(sm, oc, mag, f"band {window} {kernel}")


def _device_buffers(torch, px, guard):
    ds = torch.full((px + guard,), -77.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((px + guard,), -5, dtype=torch.int32, device="cuda:0")
    return ds, dc


@pytest.mark.parametrize("kernel", SMOOTH_KERNELS)
def test_launch_view_smooth_on_a_torch_stream(gpu, kernel):
    """mbk_view_launch_smooth, what the benchmark's cfg5 leg calls: device pointers, the caller's stream.  Whole view and
    window, with and without d_counts, on a stream that is not the default one, two launches in a row into different
    buffers before one synchronise: nu and counts equal compute_view_smooth's of the whole view, the same rows and
    columns, bit for bit; the buffer is exactly
    window-sized, and a guard region past its end keeps its sentinel (as does d_counts when it is not passed)."""
    import torch
    view, mrd = View(-2.0, -1.5, 3.0, 3.0, 600, 400), 700
    guard = 1024
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    whole_sm, whole_c, _ = gpu.compute_view_smooth(view, mrd, kernel=kernel)
    for window in (None, (37, 101, 333, 77), (0, 200, 600, 8), (599, 399, 1, 1)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        want_sm, want_c = whole_sm[r0:r0 + nr, c0:c0 + nc], whole_c[r0:r0 + nr, c0:c0 + nc]     # and so every pixel in its place
        px = want_sm.size
        bufs = [_device_buffers(torch, px, guard) for _ in range(2)]
        torch.cuda.synchronize()
        for (ds, dc), with_counts in zip(bufs, (True, False)):
            gpu.launch_view_smooth(view, mrd, d_smooth=ds.data_ptr(), d_counts=dc.data_ptr() if with_counts else 0,
                                   stream=stream.cuda_stream, window=window, kernel=kernel)
        stream.synchronize()
        for (ds, dc), with_counts in zip(bufs, (True, False)):
            hs, hc = ds.cpu().numpy(), dc.cpu().numpy()
            assert np.array_equal(hs[:px].reshape(want_sm.shape), want_sm), (window, with_counts)
            assert (hs[px:] == -77.0).all() and (hc[px:] == -5).all(), (window, with_counts)
            if with_counts:
                assert np.array_equal(hc[:px].reshape(want_c.shape), want_c), window
            else:
                assert (hc == -5).all(), window
        assert (want_c > 0).any() or window == (599, 399, 1, 1)


def test_launch_view_smooth_argument_errors(gpu):
    """As include/mbk.h states: NULL d_smooth, MBK_PRECISION_F32 and the kernels without a smooth form are
    MBK_ERR_INVALID and write nothing; mrd 0 and 1 run no step, so every count and nu is 0."""
    import torch
    view = View(-2.0, -2.0, 4.0, 4.0, 16, 16)
    cv = gpu._cview(view, None)
    ds, dc = _device_buffers(torch, 256, 64)
    torch.cuda.synchronize()
    launch = gpu._lib.mbk_view_launch_smooth
    with pytest.raises(MbkError):
        gpu.launch_view_smooth(view, 100, d_smooth=0, d_counts=dc.data_ptr())
    assert launch(gpu._h, C.byref(cv), 100, L.MBK_KERNEL_DEFAULT, dc.data_ptr(), None, None) == L.MBK_ERR_INVALID
    for kernel in ("default", "asm", "group", "scan"):
        assert launch(gpu._h, C.byref(cv), 100, L.KERNELS[kernel] | L.MBK_PRECISION_F32, dc.data_ptr(), ds.data_ptr(),
                      None) == L.MBK_ERR_INVALID, kernel
    for kernel in ("simple", "refill"):
        with pytest.raises(MbkError):
            gpu.launch_view_smooth(view, 100, d_smooth=ds.data_ptr(), d_counts=dc.data_ptr(), kernel=kernel)
        with pytest.raises(MbkError):
            gpu.compute_view_smooth(view, 100, kernel=kernel)
    with pytest.raises(MbkError):
        gpu.launch_view_smooth(view, 2 ** 31, d_smooth=ds.data_ptr())              # mrd must fit int32
    with pytest.raises(MbkError):
        gpu.launch_view_smooth(view, 100, d_smooth=ds.data_ptr(), window=(10, 0, 7, 16))    # window outside the view
    with pytest.raises(MbkError):
        gpu.launch_view_smooth(View(2.0 ** 500, 0.0, 2.0 ** 500, 1.0, 4, 4), 100, d_smooth=ds.data_ptr())   # > 2^500
    assert launch(gpu._h, None, 100, L.MBK_KERNEL_DEFAULT, None, ds.data_ptr(), None) == L.MBK_ERR_INVALID
    torch.cuda.synchronize()
    assert (ds.cpu().numpy() == -77.0).all() and (dc.cpu().numpy() == -5).all()     # no refused call wrote anything
    for mrd in (0, 1):
        for kernel in SMOOTH_KERNELS:
            ds, dc = _device_buffers(torch, 256, 64)
            torch.cuda.synchronize()
            gpu.launch_view_smooth(view, mrd, d_smooth=ds.data_ptr(), d_counts=dc.data_ptr(), kernel=kernel)
            torch.cuda.synchronize()
            hs, hc = ds.cpu().numpy(), dc.cpu().numpy()
            assert (hs[:256] == 0.0).all() and (hc[:256] == 0).all() and (hs[256:] == -77.0).all() and (hc[256:] == -5).all()
            sm, c, st = gpu.compute_view_smooth(view, mrd, kernel=kernel)
            assert not sm.any() and not c.any() and st.pixel_iterations == 0 and st.never_pixels == 256


def test_cfg5_full_size_through_launch_view_smooth(gpu, oracle):
    """BASELINE cfg5 (4096^2, mrd 5000) once through the benchmark's path: the counts hash to
    tests/golden/bench_outputs.json, the whole nu array is within the summed bound of the oracle's, and 20 000 seeded
    escaped pixels plus the 1 000 largest and the 1 000 smallest mag are within the bound of the truth."""
    import torch
    (v, mrd) = T.CFG5
    view = View(*v)
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bench_outputs.json")))["cfg5"]
    assert g["view"] == list(v) and g["mrd"] == mrd and g["window"] is None
    px = view.width * view.height
    ds, dc = _device_buffers(torch, px, 4096)
    stream = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_view_smooth(view, mrd, d_smooth=ds.data_ptr(), d_counts=dc.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    hs, hc = ds.cpu().numpy(), dc.cpu().numpy()
    assert (hs[px:] == -77.0).all() and (hc[px:] == -5).all()
    sm, c = hs[:px].reshape(view.height, view.width), hc[:px].reshape(view.height, view.width)
    assert hashlib.sha256(c.tobytes()).hexdigest() == g["counts_sha256"]
    assert int((c == 0).sum()) == g["never_pixels"]
    assert int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum()) == g["pixel_iterations"]
    osm, oc, mag = T.cfg5_oracle(oracle)
    assert np.array_equal(c, oc)
    T.assert_pair(sm, osm, oc, "cfg5 whole array")
    pick = T.cfg5_sample(oc, mag)
    T.assert_within(sm.ravel()[pick], oc.ravel()[pick], mag.ravel()[pick], "cfg5 sample")
