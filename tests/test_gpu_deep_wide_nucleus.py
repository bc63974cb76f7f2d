"""Atom periods and Newton seeds of extended-range deep views on the GPU (include/mbk.h, "Locating minibrots in extended-range
deep views"), held to the host twin (mbk_deep_xview_nucleus_host, which tests/test_deep_wide_nucleus.py holds to the numpy model
of the contract): every output bit -- count, period, delta -- of every pixel.  The views are small: what can go wrong is the
per-pixel state machine (the wide comparison, the first minimum, the escaping step, rebases, M == 1), the window arithmetic and
the argument rules, not the size.
"""
import ctypes as C

import numpy as np
import pytest

from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, WideDeepView, wide_nucleus_host
from distributedmandelbrot_amd import _lib as L
from test_deep_nucleus import CASES as PLAIN_CASES
from test_deep_nucleus import case as plain_case
from test_deep_wide_nucleus import CASES, N, SAME_AS_PLAIN, as_wide_view, case, located, round_trip, seeds_of

pytestmark = pytest.mark.gpu


def _twin(orbit, view, mrd, window=None):
    """(period [nrows, ncols], delta [nrows, ncols, 2], counts [nrows, ncols]) of the host twin"""
    c0, r0, nc, nr = window or (0, 0, view.width, view.height)
    rows, cols = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    h = wide_nucleus_host(orbit, view, (rows * view.width + cols).ravel(), mrd)
    return h["period"].reshape(nr, nc), h["delta"].reshape(nr, nc, 2), h["n"].reshape(nr, nc)


def _check(gpu, orbit, view, mrd, window=None, twin=None):
    period, delta, counts, stats = gpu.compute_wide_view_nucleus(orbit, view, mrd, window=window)
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
def test_the_two_cases_every_bit_and_a_window(gpu, name):
    orbit, view, h, _ = case(name)
    mrd = CASES[name][2]
    whole = _check(gpu, orbit, view, mrd, twin=seeds_of(h, view) + (h["n"].reshape(N, N),))
    assert (whole[0] == CASES[name][3]).any() and (whole[2] > 0).all()
    c0, r0, nc, nr = window = (3, 2, 9, 7)
    part = _check(gpu, orbit, view, mrd, window)
    for a, b in zip(part, whole):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                              (b.view(np.int64) if b.dtype == np.float64 else b)[r0:r0 + nr, c0:c0 + nc])


def test_the_edge_views(gpu):
    # the reference escapes at once: M == 1, every step starts from a rebase
    view = WideDeepView(1.0, -1000, 19, 13)
    orbit = DeepOrbit("-2", "0", 1000, min_span_exp2=view.min_span_exp2)
    assert orbit.length == 1
    _, _, counts = _check(gpu, orbit, view, 1000)
    assert (counts > 0).any()
    # a centre outside the set beside pixels inside it: the orbit runs out, the pixels rebase at m == M
    view = WideDeepView(0.8, -4, 19, 13)
    orbit = DeepOrbit("0.26", "0", 300, min_span_exp2=view.min_span_exp2)
    assert orbit.escaped and 1 < orbit.length < 100
    period, _, counts = _check(gpu, orbit, view, 300)
    assert (counts == 0).any() and (counts > orbit.length).any() and len(np.unique(period)) > 3
    # mrd below the period of the minibrot in the view; 0, 1 and 2
    view = WideDeepView(1.0, -1100, 19, 13)
    orbit = DeepOrbit("0", "1", 40, min_span_exp2=view.min_span_exp2)
    for mrd in (0, 1, 2, 40):
        period, delta, counts = _check(gpu, orbit, view, mrd)
        assert period.max() <= max(mrd, 1)
        if mrd < 2:
            assert (period == 1).all() and not counts.any()


@pytest.mark.parametrize("name", SAME_AS_PLAIN)
def test_same_bits_as_the_plain_kernel(gpu, name):
    orbit, view, _, _ = plain_case(name)
    mrd = PLAIN_CASES[name][2]
    period, delta, counts = _check(gpu, orbit, as_wide_view(view), mrd)
    pp, pd, pc, _ = gpu.compute_deep_view_nucleus(orbit, view, mrd)
    assert np.array_equal(period, pp) and np.array_equal(counts, pc)
    assert np.array_equal(delta.view(np.int64), pd.view(np.int64))


def test_launch_on_a_torch_stream_with_guards(gpu):
    import torch
    orbit, view, _, _ = case("i-2^-1100")
    mrd = CASES["i-2^-1100"][2]
    guard = 256
    stream = torch.cuda.Stream(device="cuda:0")
    wp, wd, wc, _ = gpu.compute_wide_view_nucleus(orbit, view, mrd)
    for window in (None, (3, 2, 9, 7)):
        c0, r0, nc, nr = window or (0, 0, view.width, view.height)
        px = nc * nr
        for with_counts in (True, False):
            dp = torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
            dc = torch.full((px + 2 * guard,), -6, dtype=torch.int32, device="cuda:0")
            dd = torch.full((2 * px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            gpu.launch_wide_view_nucleus(orbit, view, mrd, d_period=dp[guard:].data_ptr(), d_delta=dd[guard:].data_ptr(),
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
    view = WideDeepView(1.0, -1100, 16, 16)
    orbit = DeepOrbit("0", "1", 500, min_span_exp2=view.min_span_exp2)
    cv = gpu._cdeep(view, None)
    dp = torch.full((256,), -5, dtype=torch.int32, device="cuda:0")
    dc = torch.full((256,), -6, dtype=torch.int32, device="cuda:0")
    dd = torch.full((512,), -77.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    pp, pc, pd = dp.data_ptr(), dc.data_ptr(), dd.data_ptr()
    hp, hc, hd = np.full(256, -5, np.int32), np.full(256, -6, np.int32), np.full(512, -77.0)
    launch, compute = gpu._lib.mbk_deep_xview_launch_nucleus, gpu._lib.mbk_deep_xview_compute_nucleus

    def refused(flags=0, o=orbit._h, v=C.byref(cv), mrd=100, period=True, delta=True, text=None):
        for rc in (launch(gpu._h, o, v, mrd, flags, pc, pp if period else None, pd if delta else None, None),
                   compute(gpu._h, o, v, mrd, flags, hc.ctypes.data, hp.ctypes.data if period else None,
                           hd.ctypes.data if delta else None, None)):
            assert rc == L.MBK_ERR_INVALID
            if text:
                assert text in gpu._lib.mbk_last_error(gpu._h).decode()

    refused(flags=L.MBK_DEEP_XBLA, text="MBK_DEEP_XBLA is not implemented for atom periods (a skipped run has no |z_n| to compare)")
    refused(flags=L.MBK_DEEP_BLA, text="MBK_DEEP_BLA is not implemented for extended-range deep views")
    for flags in (L.KERNELS["asm"], L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_WANT_COUNTS, L.MBK_WANT_BYTES):
        refused(flags=flags, text="no flags")
    refused(period=False, text="NULL period or delta pointer")
    refused(delta=False, text="NULL period or delta pointer")
    refused(o=None)
    refused(v=None)
    refused(mrd=501, text="mrd exceeds")                                 # above the orbit's
    for rng, exp2 in ((2.0 ** -65, -1100), (4.5, -1100), (float("nan"), -1100), (1.0, 1), (1.0, -8193)):
        bad = gpu._cdeep(WideDeepView(rng, exp2, 16, 16), None)
        refused(v=C.byref(bad))
    bad = gpu._cdeep(view, (10, 0, 7, 16))                              # the window exceeds the view
    refused(v=C.byref(bad), text="window exceeds the view")
    plain = DeepView(1e-20, 16, 16)
    with pytest.raises(ValueError):
        gpu.compute_wide_view_nucleus(orbit, plain, 100)
    with pytest.raises(ValueError):
        gpu.launch_wide_view_nucleus(orbit, plain, 100, d_period=pp, d_delta=pd)
    with pytest.raises(ValueError):
        gpu.locate_wide_nucleus(orbit, plain, 100)
    with pytest.raises(MbkError):
        gpu.launch_wide_view_nucleus(orbit, view, 100, d_period=0, d_delta=pd)
    with pytest.raises(ValueError):                                      # the plain calls keep refusing a WideDeepView
        gpu.compute_deep_view_nucleus(orbit, view, 100)
    torch.cuda.synchronize()
    assert (dp.cpu().numpy() == -5).all() and (dc.cpu().numpy() == -6).all() and (dd.cpu().numpy() == -77.0).all()
    assert (hp == -5).all() and (hc == -6).all() and (hd == -77.0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_locate_wide_nucleus_end_to_end(gpu, name):
    orbit, view, _, _ = case(name)
    want = located(name)                     # the CPU path, on host-twin arrays
    nuc = gpu.locate_wide_nucleus(orbit, view, CASES[name][2])
    assert nuc == want and nuc.period == CASES[name][3] and nuc.inside is True
    v = nuc.view(17)
    assert isinstance(v, WideDeepView)
    mrd = 4 * nuc.period
    counts, _, _, _ = gpu.compute_deep_view(nuc.orbit(mrd), v, mrd, want_bytes=False)
    assert counts[8, 8] == 0


def test_round_trip_on_the_device(gpu):
    first, orbit, view, _, want = round_trip()
    nuc = gpu.locate_wide_nucleus(orbit, view, 4 * first.period)
    assert nuc == want and nuc.period == first.period == 534
