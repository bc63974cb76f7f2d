"""Atom periods and Newton seeds on the GPU (include/mbk.h, "Locating minibrots in deep views"), held to the host twin
(mbk_deep_nucleus_host, which tests/test_deep_nucleus.py holds to the numpy model of the contract): every output bit -- count,
period, delta -- of every pixel.  The views are small: what can go wrong is the per-pixel state machine (first minimum, the
escaping step, rebases, M == 1, the rescaled derivative), the window arithmetic and the argument rules, not the size.
"""
import ctypes as C

import numpy as np
import pytest

from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, WideDeepView, deep_nucleus_host
from distributedmandelbrot_amd import _lib as L
from test_deep_nucleus import CASES, N, case, located

pytestmark = pytest.mark.gpu


def _twin(orbit, view, mrd, window=None):
    """(period [nrows, ncols], delta [nrows, ncols, 2], counts [nrows, ncols]) of the host twin"""
    c0, r0, nc, nr = window or (0, 0, view.width, view.height)
    rows, cols = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    h = deep_nucleus_host(orbit, view, (rows * view.width + cols).ravel(), mrd)
    return h["period"].reshape(nr, nc), h["delta"].reshape(nr, nc, 2), h["n"].reshape(nr, nc)


def _check(gpu, orbit, view, mrd, window=None, twin=None):
    period, delta, counts, stats = gpu.compute_deep_view_nucleus(orbit, view, mrd, window=window)
    wp, wd, wc = twin if twin is not None else _twin(orbit, view, mrd, window)
    assert period.dtype == np.int32 and delta.dtype == np.float64 and counts.dtype == np.int32
    assert period.shape == wp.shape and delta.shape == wd.shape
    assert np.array_equal(counts, wc), int((counts != wc).sum())
    assert np.array_equal(period, wp), int((period != wp).sum())
    assert np.array_equal(delta.view(np.int64), wd.view(np.int64)), int((delta.view(np.int64) != wd.view(np.int64)).sum())
    ref, _, _, _ = gpu.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False)
    assert np.array_equal(counts, ref)
    assert stats.pixel_iterations == int(np.where(counts > 0, counts, max(mrd - 1, 0)).astype(np.int64).sum())
    assert stats.never_pixels == int((counts == 0).sum())
    return period, delta, counts


@pytest.mark.parametrize("name", list(CASES))
def test_the_three_cases_every_bit(gpu, name):
    orbit, view, h, _ = case(name)
    period, _, counts = _check(gpu, orbit, view, CASES[name][2],
                               twin=(h["period"].reshape(N, N), h["delta"].reshape(N, N, 2), h["n"].reshape(N, N)))
    assert (period == CASES[name][3]).any() and (counts > 0).all()


def test_partial_blocks_and_windows(gpu):
    centre, span, mrd, _, _ = CASES["i-1e-20"]
    orbit = case("i-1e-20")[0]
    _check(gpu, orbit, DeepView(span, 19, 13), mrd)
    view = DeepView(span, 40, 24)
    whole = _check(gpu, orbit, view, mrd)
    for window in ((5, 3, 21, 11), (39, 23, 1, 1), (8, 16, 32, 8)):
        c0, r0, nc, nr = window
        part = _check(gpu, orbit, view, mrd, window)
        for a, b in zip(part, whole):
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                  (b.view(np.int64) if b.dtype == np.float64 else b)[r0:r0 + nr, c0:c0 + nc]), window


def test_short_orbits_and_shallow_mrd(gpu):
    # the reference escapes at once: M == 1, every step starts from a rebase
    orbit = DeepOrbit("-2", "0", 1000, min_span=1e-10)
    assert orbit.length == 1
    _, _, counts = _check(gpu, orbit, DeepView(1e-10, 16, 16), 1000)
    assert (counts > 0).any()
    # a centre outside the set beside pixels inside it: the orbit runs out, the pixels rebase at m == M
    orbit = DeepOrbit("0.26", "0", 300, min_span=0.05)
    assert orbit.escaped and 1 < orbit.length < 100
    period, _, counts = _check(gpu, orbit, DeepView(0.05, 16, 16), 300)
    assert (counts == 0).any() and (counts > orbit.length).any() and len(np.unique(period)) > 3
    # mrd below the period of the minibrot in the view; 0, 1 and 2
    orbit, view, _, _ = case("i-1e-20")
    period, _, _ = _check(gpu, orbit, view, 40)
    assert period.max() <= 40
    for mrd in (0, 1, 2):
        period, delta, counts = _check(gpu, orbit, view, mrd)
        if mrd < 2:
            assert (period == 1).all() and not counts.any()


def test_launch_on_a_torch_stream_with_guards(gpu):
    import torch
    orbit, view, _, _ = case("i-1e-200")
    mrd = CASES["i-1e-200"][2]
    guard = 256
    stream = torch.cuda.Stream(device="cuda:0")
    wp, wd, wc, _ = gpu.compute_deep_view_nucleus(orbit, view, mrd)
    for window in (None, (3, 5, 11, 9)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        px = nc * nr
        for with_counts in (True, False):
            dp = torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
            dc = torch.full((px + 2 * guard,), -6, dtype=torch.int32, device="cuda:0")
            dd = torch.full((2 * px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            gpu.launch_deep_view_nucleus(orbit, view, mrd, d_period=dp[guard:].data_ptr(), d_delta=dd[guard:].data_ptr(),
                                         d_counts=dc[guard:].data_ptr() if with_counts else 0, stream=stream.cuda_stream, window=window)
            stream.synchronize()
            hp, hc, hd = dp.cpu().numpy(), dc.cpu().numpy(), dd.cpu().numpy()
            assert np.array_equal(hp[guard:guard + px].reshape(nr, nc), wp[r0:r0 + nr, c0:c0 + nc]), (window, with_counts)
            assert np.array_equal(hd[guard:guard + 2 * px].reshape(nr, nc, 2).view(np.int64),
                                  wd[r0:r0 + nr, c0:c0 + nc].copy().view(np.int64)), (window, with_counts)
            assert (hp[:guard] == -5).all() and (hp[guard + px:] == -5).all()
            assert (hd[:guard] == -77.0).all() and (hd[guard + 2 * px:] == -77.0).all()
            assert (hc[:guard] == -6).all() and (hc[guard + px:] == -6).all()
            if with_counts:
                assert np.array_equal(hc[guard:guard + px].reshape(nr, nc), wc[r0:r0 + nr, c0:c0 + nc]), window
            else:
                assert (hc == -6).all()


def test_refusals_write_nothing(gpu):
    import torch
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    view = DeepView(1e-20, 16, 16)
    cv = gpu._cdeep(view, None)
    dp = torch.full((256,), -5, dtype=torch.int32, device="cuda:0")
    dc = torch.full((256,), -6, dtype=torch.int32, device="cuda:0")
    dd = torch.full((512,), -77.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    pp, pc, pd = dp.data_ptr(), dc.data_ptr(), dd.data_ptr()
    hp, hc, hd = np.full(256, -5, np.int32), np.full(256, -6, np.int32), np.full(512, -77.0)
    launch, compute = gpu._lib.mbk_deep_view_launch_nucleus, gpu._lib.mbk_deep_view_compute_nucleus

    def refused(flags=0, o=orbit._h, v=C.byref(cv), mrd=100, period=True, delta=True, text=None):
        for rc in (launch(gpu._h, o, v, mrd, flags, pc, pp if period else None, pd if delta else None, None),
                   compute(gpu._h, o, v, mrd, flags, hc.ctypes.data, hp.ctypes.data if period else None,
                           hd.ctypes.data if delta else None, None)):
            assert rc == L.MBK_ERR_INVALID
            if text:
                assert text in gpu._lib.mbk_last_error(gpu._h).decode()

    refused(flags=L.MBK_DEEP_BLA, text="a skipped run has no |z_n| to compare")
    for flags in (L.MBK_DEEP_XBLA, L.KERNELS["asm"], L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_WANT_COUNTS):
        refused(flags=flags, text="no flags")
    refused(period=False)
    refused(delta=False)
    refused(o=None)
    refused(v=None)
    refused(mrd=501)                                                    # above the orbit's
    for span in (2.0 ** -961, 4.5, float("nan")):
        bad = gpu._cdeep(DeepView(span, 16, 16), None)
        refused(v=C.byref(bad))
    bad = gpu._cdeep(view, (10, 0, 7, 16))                              # the window exceeds the view
    refused(v=C.byref(bad))
    wide = WideDeepView(0.5, -1000, 16, 16)
    with pytest.raises(ValueError):
        gpu.compute_deep_view_nucleus(orbit, wide, 100)
    with pytest.raises(ValueError):
        gpu.launch_deep_view_nucleus(orbit, wide, 100, d_period=pp, d_delta=pd)
    with pytest.raises(ValueError):
        gpu.locate_nucleus(orbit, wide, 100)
    with pytest.raises(MbkError):
        gpu.launch_deep_view_nucleus(orbit, view, 100, d_period=0, d_delta=pd)
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == -5).all() and (dc.cpu().numpy() == -6).all() and (dd.cpu().numpy() == -77.0).all()
    assert (hp == -5).all() and (hc == -6).all() and (hd == -77.0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_locate_nucleus_end_to_end(gpu, name):
    orbit, view, _, _ = case(name)
    want = located(name)                     # the CPU path, on host-twin arrays
    nuc = gpu.locate_nucleus(orbit, view, CASES[name][2])
    assert nuc == want and (nuc.center_r, nuc.center_i, nuc.period) == (want.center_r, want.center_i, CASES[name][3])
    v = nuc.view(17, 17)
    assert isinstance(v, WideDeepView) == (name == "i-1e-200")
    mrd = 16 * nuc.period
    counts, _, _, _ = gpu.compute_deep_view(nuc.orbit(mrd), v, mrd, want_bytes=False)
    assert counts[8, 8] == 0
    assert all(counts[r, c] > 0 for r, c in ((0, 0), (0, 16), (16, 0), (16, 16)))
