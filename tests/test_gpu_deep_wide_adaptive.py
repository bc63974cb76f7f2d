"""Adaptive supersampling of extended-range deep views on the GPU (include/mbk.h, the section of that name): image, mask and
statistics are held bit for bit to the numpy restatement of the adaptive contract (tests/adaptive_model.py) applied to the
samples the same device returns for the wide view and for the s times finer wide view -- with the plain wide step and with
MBK_DEEP_XBLA, where base and fine samples step with the tables of two different dcmax --, as tests/test_gpu_deep_adaptive.py
holds the deep views; thresholds 0 and 256 also to render_deep_view itself."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as A
import deep_wide_adaptive_cases as K
import deep_wide_bla_model as X
import deep_wide_model as W
import render_model as M
from distributedmandelbrot_amd import DeepView, MbkError, WideDeepView
from distributedmandelbrot_amd import _lib as L

pytestmark = pytest.mark.gpu

_cache = {}


def _samples(gpu, name, s, xbla):
    """(nu, counts) of the case's view at s times the resolution, from the device; computed once and left unchanged."""
    if (name, s, xbla) not in _cache:
        orbit, view, mrd, _, _ = K.case(name)
        counts, _, nu, _ = gpu.compute_deep_view(orbit, K.finer(view, s), mrd, want_bytes=False, want_smooth=True, xbla=xbla)
        nu.setflags(write=False)
        counts.setflags(write=False)
        _cache[name, s, xbla] = (nu, counts)
    return _cache[name, s, xbla]


def _model(gpu, name, s, thr, xbla):
    pal = K.case(name)[3]
    bn, bc = _samples(gpu, name, 1, xbla)
    fn, fc = _samples(gpu, name, s, xbla)
    return A.render_adaptive(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, bc, bn, fc, fn)


def _stats_model(gpu, name, s, mask, xbla, window=None):
    mrd = K.case(name)[2]
    return A.sample_stats(mask, mrd, s, _samples(gpu, name, 1, xbla)[1], _samples(gpu, name, s, xbla)[1], window)


@pytest.mark.parametrize("xbla", [False, True], ids=["plain", "xbla"])
@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("name", list(K.CASES))
def test_image_mask_and_statistics_equal_the_model_on_the_devices_own_samples(gpu, name, s, xbla):
    orbit, view, mrd, pal, mid = K.case(name)
    w, h = view.width, view.height
    for thr in (0, mid, 256):
        want, want_mask = _model(gpu, name, s, thr, xbla)
        share = want_mask.mean()
        print(name, s, xbla, thr, "refined share of the model's mask:", share)
        if thr == mid:
            assert 0.05 <= share <= 0.60, share      # neither an empty nor a full list
        img, mask, st = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=thr, want_mask=True,
                                                      xbla=xbla)
        assert img.shape == (h, w, 4) and img.dtype == np.uint8 and mask.shape == (h, w) and mask.dtype == np.uint8
        assert np.array_equal(mask, want_mask), (thr, int((mask != want_mask).sum()))
        assert np.array_equal(img, want), (thr, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, want_mask, xbla), thr
        assert st.kernel_ms > 0
        # without a mask: the same image
        img2, _ = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=thr, xbla=xbla)
        assert np.array_equal(img2, img), thr
        if thr == 0:
            full, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, supersample=s, xbla=xbla)
            assert mask.all() and np.array_equal(img, full)
        if thr == 256 or s == 1:
            one, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, supersample=1, xbla=xbla)
            assert (thr < 256 or not mask.any()) and np.array_equal(img, one)


@pytest.mark.parametrize("name", [n for n in K.CASES if K.CASES[n][2] <= -1100])
def test_the_xbla_samples_are_not_the_plain_ones(gpu, name):
    """What keeps the xbla cases above from passing on the plain step: nu differs in bits on some pixels."""
    assert not np.array_equal(_samples(gpu, name, 1, True)[0], _samples(gpu, name, 1, False)[0])


def test_an_orbit_of_length_one_takes_the_plain_step_whatever_the_flag(gpu):
    mrd = 200
    view = K.wide_view(1.0, -1100, 40, 24)
    orbit = K.orbit(("-2", "0"), mrd, view.min_span_exp2)
    assert orbit.length == 1
    for s in (2, 3, 8):
        want, _ = gpu.render_deep_view(orbit, view, mrd, palette=K.PAL, supersample=s)
        for xbla in (False, True):
            img, mask, _ = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=K.PAL, supersample=s, threshold=0, want_mask=True,
                                                         xbla=xbla)
            assert mask.all() and np.array_equal(img, want), (s, xbla)


def test_a_view_inside_the_set_refines_nothing(gpu):
    mrd, (w, h) = 200, (67, 45)
    view = K.wide_view(1.0, -1100, w, h)
    orbit = K.orbit(("0", "0"), mrd, view.min_span_exp2)
    for s in (2, 8):
        for xbla in (False, True):
            img, mask, st = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=K.PAL, supersample=s, threshold=1, want_mask=True,
                                                          xbla=xbla)
            assert not mask.any()
            assert (img == np.array(K.PAL.inside, np.uint8)).all()
            assert (st.pixel_iterations, st.never_pixels) == (w * h * (mrd - 1), w * h)


# odd offsets, touching the right and the top edge of the view; touching no edge.  The first is test_gpu_adaptive.py's for a
# view 67 wide; at the 65 columns of i-1100-two-tables the same 22 x 14 window is moved left until it touches the right edge again.
WINDOWS = [(45, 31, 22, 14), (3, 5, 31, 17)]


def _windows(view):
    return [(view.width - nc if c0 + nc > view.width else c0, r0, nc, nr) for c0, r0, nc, nr in WINDOWS]


@pytest.mark.parametrize("name, xbla", [("i-1100", False), ("i-1100-two-tables", True)])
def test_windows_and_bands_equal_the_same_rectangle_of_the_whole_image(gpu, name, xbla):
    s = 3
    orbit, view, mrd, pal, mid = K.case(name)
    whole, whole_mask = _model(gpu, name, s, mid, xbla)
    for window in _windows(view):
        c0, r0, nc, nr = window
        assert c0 % 2 == 1 and r0 % 2 == 1 and c0 + nc <= view.width and r0 + nr <= view.height
        for rows in (0, 4):
            img, mask, st = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid, window=window,
                                                          max_band_rows=rows, want_mask=True, xbla=xbla)
            assert np.array_equal(img, whole[r0:r0 + nr, c0:c0 + nc]), (window, rows)
            assert np.array_equal(mask, whole_mask[r0:r0 + nr, c0:c0 + nc]), (window, rows)
            # the halo is not counted, and nothing twice across bands
            assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, whole_mask, xbla, window), (window, rows)
    # the halo crosses bands: band heights of 1 and 5 give the unbanded image
    for s in (2, 8):
        whole, whole_mask = _model(gpu, name, s, mid, xbla)
        for rows in (1, 5):
            img, mask, st = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid,
                                                          max_band_rows=rows, want_mask=True, xbla=xbla)
            assert np.array_equal(img, whole) and np.array_equal(mask, whole_mask), (s, rows)
            assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, whole_mask, xbla), (s, rows)


# One listed pixel is a list shorter than one group of the refine kernel's walk at s = 2, 3, 4 (16, 7, 4 pixels to a group) and
# three end inside a group; at s = 8 a pixel is a group.  Inside the 67 x 45 view; touching its right and its bottom edge.
TINY_WINDOWS = [(33, 22, 1, 1), (64, 44, 3, 1)]


@pytest.mark.parametrize("xbla", [False, True], ids=["plain", "xbla"])
@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_lists_shorter_than_a_group_equal_the_same_pixels_of_the_full_render(gpu, s, xbla):
    name = "i-1100"
    orbit, view, mrd, pal, _ = K.case(name)
    full, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, supersample=s, xbla=xbla)
    everything = np.ones((view.height, view.width), bool)
    for window in TINY_WINDOWS:
        c0, r0, nc, nr = window
        img, st = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=0, window=window, xbla=xbla)
        assert np.array_equal(img, full[r0:r0 + nr, c0:c0 + nc]), window
        assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, everything, xbla, window), window


def test_both_tables_of_a_render_stay_resident_and_a_third_span_takes_only_one_place(gpu):
    """Three dcmax in turn on one orbit (the two of an adaptive render, then a count launch's, then the two again) and another
    orbit's render in between: every result is its model's, and the first render comes back bit for bit."""
    first, second = ("i-1100-two-tables", 2), ("i-3000-two-tables", 3)
    got = []
    for name, s in (first, second, (None, 0), first):
        if name is None:
            orbit, _, mrd, _, _ = K.case(first[0])
            third = K.wide_view(1.0, -1000, 48, 40)
            xr, xi, xe = orbit.wide_table()
            mc, _, _ = X.counts(xr, xi, xe, *W.offsets(third), third.exp2, mrd, X.build(xr, xi, xe, X.dcmax(third)))
            c, _, _, _ = gpu.compute_deep_view(orbit, third, mrd, want_bytes=False, xbla=True)
            assert np.array_equal(c.ravel(), mc)
            continue
        orbit, view, mrd, pal, mid = K.case(name)
        assert X.dcmax(view) != X.dcmax(K.finer(view, s))
        img, mask, st = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid, want_mask=True,
                                                      xbla=True)
        got.append((img, mask, (st.pixel_iterations, st.never_pixels)))
    for (img, mask, st), (name, s) in zip(got, (first, second, first)):
        want, want_mask = _model(gpu, name, s, K.case(name)[4], True)
        assert np.array_equal(img, want) and np.array_equal(mask, want_mask), name
        assert st == _stats_model(gpu, name, s, want_mask, True), name
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1]) and got[0][2] == got[2][2]


@pytest.mark.parametrize("xbla", [False, True], ids=["plain", "xbla"])
def test_launch_on_a_torch_buffer_and_stream_equals_the_compute_form(gpu, xbla):
    import torch
    orbit, view, mrd, pal, mid = K.case("i-1100-two-tables")
    guard = 4096
    stream = torch.cuda.Stream()
    for s, window in [(2, None), (4, (19, 15, 22, 14))]:      # (the window holds the centre pixel and the edges around it)
        want, want_mask, _ = gpu.render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid, window=window,
                                                           want_mask=True, xbla=xbla)
        assert 0 < int(want_mask.sum()) < want_mask.size
        n, m = want.size, want_mask.size
        for with_mask in (True, False):
            buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            mbuf = torch.full((guard + m + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                gpu.launch_render_wide_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid,
                                                     d_rgba=buf.data_ptr() + guard,
                                                     d_mask=mbuf.data_ptr() + guard if with_mask else 0,
                                                     stream=stream.cuda_stream, window=window, max_band_rows=7, xbla=xbla)
            stream.synchronize()
            got, gotm = buf.cpu().numpy(), mbuf.cpu().numpy()
            assert np.array_equal(got[guard:guard + n].reshape(want.shape), want), (s, with_mask)
            assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all(), (s, with_mask)
            if with_mask:
                assert np.array_equal(gotm[guard:guard + m].reshape(want_mask.shape), want_mask), s
                assert (gotm[:guard] == 0xA5).all() and (gotm[guard + m:] == 0xA5).all(), s
            else:
                assert (gotm == 0xA5).all()


def test_refusals_leave_the_outputs_untouched(gpu):
    lib = L.load()
    mrd = 3000
    view = K.wide_view(1.0, -1100, 64, 48)
    orbit = K.orbit(("0", "1"), mrd, view.min_span_exp2)
    pal2 = np.zeros((2, 4), np.uint8)
    pal256 = np.zeros((256, 4), np.uint8)
    out = np.full((48, 64, 4), 0xA5, np.uint8)
    mask = np.full((48, 64), 0xA5, np.uint8)

    def spec(source=L.MBK_RENDER_SMOOTH, s=2, pal=pal2, scale=1.0):
        return L.mbk_render_spec(source, s, pal.ctypes.data if pal is not None else None, 2 if pal is None else len(pal),
                                 (C.c_uint8 * 4)(0, 0, 0, 255), scale, 0.0, 0)

    def call(sp, thr=17, cv=False, mrd=mrd, flags=0, dst=out, orb=orbit._h):
        cv = gpu._cdeep(view, None) if cv is False else cv
        st = lib.mbk_deep_xview_render_adaptive_compute(gpu._h, orb, C.byref(cv) if cv is not None else None, mrd, flags,
                                                        C.byref(sp) if sp is not None else None, thr,
                                                        dst.ctypes.data if dst is not None else None, mask.ctypes.data, None)
        assert (out == 0xA5).all() and (mask == 0xA5).all()
        return st

    big = WideDeepView(1.0, -1100, 2 ** 29, 48, 1.0)
    positive = gpu._cdeep(view, None)
    positive.exp2 = 1
    cases = {
        "threshold 257": lambda: call(spec(), thr=257),
        "threshold 2^32 - 1": lambda: call(spec(), thr=2 ** 32 - 1),
        "bytes": lambda: call(spec(source=L.MBK_RENDER_BYTES, pal=pal256)),
        "equalized": lambda: call(spec(source=L.MBK_RENDER_EQUALIZED)),
        "distance": lambda: call(spec(source=L.MBK_RENDER_DISTANCE)),
        "distance_rel": lambda: call(spec(source=L.MBK_RENDER_DISTANCE_REL)),
        "MBK_DEEP_BLA": lambda: call(spec(), flags=L.MBK_DEEP_BLA),
        "MBK_DEEP_BLA beside MBK_DEEP_XBLA": lambda: call(spec(), flags=L.MBK_DEEP_BLA | L.MBK_DEEP_XBLA),
        "a kernel selector": lambda: call(spec(), flags=L.MBK_KERNEL_ASM),
        "fp32": lambda: call(spec(), flags=L.MBK_PRECISION_F32),
        "an output flag": lambda: call(spec(), flags=L.MBK_WANT_COUNTS),
        "NULL orbit": lambda: call(spec(), orb=None),
        "NULL view": lambda: call(spec(), cv=None),
        "NULL spec": lambda: call(None),
        "NULL palette": lambda: call(spec(pal=None)),
        "NULL output": lambda: call(spec(), dst=None),
        "s = 5": lambda: call(spec(s=5)),
        "mrd above the orbit's": lambda: call(spec(), mrd=mrd + 1),
        "window exceeds the view": lambda: call(spec(), cv=gpu._cdeep(view, (1, 0, 64, 48))),
        "empty window": lambda: call(spec(), cv=gpu._cdeep(view, (0, 0, 0, 48))),
        "exp2 = 1": lambda: call(spec(), cv=positive),
        "W s overflows": lambda: call(spec(s=8), cv=gpu._cdeep(big, (0, 0, 64, 48))),
    }
    for name, case in cases.items():
        assert case() == L.MBK_ERR_INVALID, name
    for flags in (L.MBK_DEEP_BLA, L.MBK_DEEP_BLA | L.MBK_DEEP_XBLA):
        assert call(spec(), flags=flags) == L.MBK_ERR_INVALID
        assert lib.mbk_last_error(gpu._h) == b"MBK_DEEP_BLA is not implemented for extended-range deep views"   # validate_deep_wide's
    with pytest.raises(MbkError):
        gpu.render_wide_view_adaptive(orbit, view, mrd, palette=K.PAL, supersample=2, threshold=257)
    with pytest.raises(ValueError):
        gpu.render_wide_view_adaptive(orbit, DeepView(1e-100, 64, 48), mrd, palette=K.PAL, supersample=2, threshold=17)
    with pytest.raises(ValueError):
        gpu.launch_render_wide_view_adaptive(orbit, DeepView(1e-100, 64, 48), mrd, palette=K.PAL, supersample=2, threshold=17,
                                             d_rgba=out.ctypes.data)

    # the launch form refuses the same way: device buffers stay as they were
    import torch
    buf = torch.full((48 * 64 * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
    mbuf = torch.full((48 * 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cv = gpu._cdeep(view, None)
    for sp, thr, flags in ((spec(), 257, 0), (spec(source=L.MBK_RENDER_BYTES, pal=pal256), 17, 0), (spec(), 17, L.MBK_DEEP_BLA),
                           (spec(), 17, L.MBK_KERNEL_ASM)):
        assert lib.mbk_deep_xview_render_adaptive_launch(gpu._h, orbit._h, C.byref(cv), mrd, flags, C.byref(sp), thr, buf.data_ptr(),
                                                         mbuf.data_ptr(), None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_render_adaptive_launch(gpu._h, orbit._h, C.byref(cv), mrd, 0, C.byref(spec()), 17, None,
                                                     mbuf.data_ptr(), None) == L.MBK_ERR_INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all() and (mbuf.cpu().numpy() == 0x5A).all()
    # and a good call works afterwards
    ok = np.empty((48, 64, 4), np.uint8)
    for flags in (0, L.MBK_DEEP_XBLA):
        assert lib.mbk_deep_xview_render_adaptive_compute(gpu._h, orbit._h, C.byref(cv), mrd, flags, C.byref(spec()), 17,
                                                          ok.ctypes.data, None, None) == L.MBK_OK
