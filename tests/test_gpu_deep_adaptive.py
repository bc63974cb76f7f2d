"""Adaptive supersampling of deep views on the GPU (include/mbk.h, the section of that name): image, mask and statistics are
held bit for bit to the numpy restatement of the adaptive contract (tests/adaptive_model.py) applied to the samples the same
device returns for the view and for the s times finer view -- with the plain step and with MBK_DEEP_BLA, where base and fine
samples step with the tables of two different dcmax --, as tests/test_gpu_adaptive.py holds the plain views; thresholds 0 and
256 also to render_deep_view itself."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as A
import deep_adaptive_cases as K
import deep_bla_model as B
import deep_model as D
import render_model as M
from distributedmandelbrot_amd import DeepView, MbkError, WideDeepView
from distributedmandelbrot_amd import _lib as L

pytestmark = pytest.mark.gpu

_cache = {}


def _samples(gpu, name, s, bla):
    """(nu, counts) of the case's view at s times the resolution, from the device; computed once and left unchanged."""
    if (name, s, bla) not in _cache:
        orbit, view, mrd, _, _ = K.case(name)
        counts, _, nu, _ = gpu.compute_deep_view(orbit, K.finer(view, s), mrd, want_bytes=False, want_smooth=True, bla=bla)
        nu.setflags(write=False)
        counts.setflags(write=False)
        _cache[name, s, bla] = (nu, counts)
    return _cache[name, s, bla]


def _model(gpu, name, s, thr, bla):
    pal = K.case(name)[3]
    bn, bc = _samples(gpu, name, 1, bla)
    fn, fc = _samples(gpu, name, s, bla)
    return A.render_adaptive(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, bc, bn, fc, fn)


def _stats_model(gpu, name, s, mask, bla, window=None):
    mrd = K.case(name)[2]
    return A.sample_stats(mask, mrd, s, _samples(gpu, name, 1, bla)[1], _samples(gpu, name, s, bla)[1], window)


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("name", list(K.CASES))
def test_image_mask_and_statistics_equal_the_model_on_the_devices_own_samples(gpu, name, s, bla):
    orbit, view, mrd, pal, mid = K.case(name)
    w, h = view.width, view.height
    for thr in (0, mid, 256):
        want, want_mask = _model(gpu, name, s, thr, bla)
        share = want_mask.mean()
        print(name, s, bla, thr, "refined share of the model's mask:", share)
        if thr == mid:
            assert 0.05 <= share <= 0.60, share      # neither an empty nor a full list
        img, mask, st = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=thr, want_mask=True,
                                                      bla=bla)
        assert img.shape == (h, w, 4) and img.dtype == np.uint8 and mask.shape == (h, w) and mask.dtype == np.uint8
        assert np.array_equal(mask, want_mask), (thr, int((mask != want_mask).sum()))
        assert np.array_equal(img, want), (thr, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, want_mask, bla), thr
        assert st.kernel_ms > 0
        # without a mask: the same image
        img2, _ = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=thr, bla=bla)
        assert np.array_equal(img2, img), thr
        if thr == 0:
            full, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, supersample=s, bla=bla)
            assert mask.all() and np.array_equal(img, full)
        if thr == 256 or s == 1:
            one, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, supersample=1, bla=bla)
            assert (thr < 256 or not mask.any()) and np.array_equal(img, one)


def test_an_orbit_of_length_one_takes_the_plain_step_whatever_the_flag(gpu):
    mrd = 200
    orbit = K.orbit(("-2", "0"), mrd, 1e-60)
    assert orbit.length == 1
    view = DeepView(1e-60, 40, 24, 1e-60 * 24 / 40)
    for s in (2, 3, 8):
        want, _ = gpu.render_deep_view(orbit, view, mrd, palette=K.PAL, supersample=s)
        for bla in (False, True):
            img, mask, _ = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=K.PAL, supersample=s, threshold=0, want_mask=True,
                                                         bla=bla)
            assert mask.all() and np.array_equal(img, want), (s, bla)


def test_a_view_inside_the_set_refines_nothing(gpu):
    mrd, (w, h) = 200, (67, 45)
    orbit = K.orbit(("0", "0"), mrd, 1e-30)
    view = DeepView(1e-30, w, h, 1e-30 * h / w)
    for s in (2, 8):
        for bla in (False, True):
            img, mask, st = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=K.PAL, supersample=s, threshold=1, want_mask=True,
                                                          bla=bla)
            assert not mask.any()
            assert (img == np.array(K.PAL.inside, np.uint8)).all()
            assert (st.pixel_iterations, st.never_pixels) == (w * h * (mrd - 1), w * h)


# odd offsets, touching the right and the top edge of the view; touching no edge.  The first is test_gpu_adaptive.py's for a
# view 67 wide; at the 59 columns of i-30-two-tables the same 22 x 14 window is moved left until it touches the right edge again.
WINDOWS = [(45, 31, 22, 14), (3, 5, 31, 17)]


def _windows(view):
    return [(view.width - nc if c0 + nc > view.width else c0, r0, nc, nr) for c0, r0, nc, nr in WINDOWS]


@pytest.mark.parametrize("name, bla", [("i-30", False), ("i-30-two-tables", True)])
def test_windows_and_bands_equal_the_same_rectangle_of_the_whole_image(gpu, name, bla):
    s = 3
    orbit, view, mrd, pal, mid = K.case(name)
    whole, whole_mask = _model(gpu, name, s, mid, bla)
    for window in _windows(view):
        c0, r0, nc, nr = window
        assert c0 % 2 == 1 and r0 % 2 == 1 and c0 + nc <= view.width and r0 + nr <= view.height
        for rows in (0, 4):
            img, mask, st = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid, window=window,
                                                          max_band_rows=rows, want_mask=True, bla=bla)
            assert np.array_equal(img, whole[r0:r0 + nr, c0:c0 + nc]), (window, rows)
            assert np.array_equal(mask, whole_mask[r0:r0 + nr, c0:c0 + nc]), (window, rows)
            # the halo is not counted, and nothing twice across bands
            assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, whole_mask, bla, window), (window, rows)
    # the halo crosses bands: band heights of 1 and 5 give the unbanded image
    for s in (2, 8):
        whole, whole_mask = _model(gpu, name, s, mid, bla)
        for rows in (1, 5):
            img, mask, st = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid,
                                                          max_band_rows=rows, want_mask=True, bla=bla)
            assert np.array_equal(img, whole) and np.array_equal(mask, whole_mask), (s, rows)
            assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, whole_mask, bla), (s, rows)


# One listed pixel is a list shorter than one group of the refine kernel's walk at s = 2, 3, 4 (16, 7, 4 pixels to a group) and
# three end inside a group; at s = 8 a pixel is a group.  Inside the 67 x 45 view; touching its right and its bottom edge.
TINY_WINDOWS = [(33, 22, 1, 1), (64, 44, 3, 1)]


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_lists_shorter_than_a_group_equal_the_same_pixels_of_the_full_render(gpu, s, bla):
    name = "i-30"
    orbit, view, mrd, pal, _ = K.case(name)
    full, _ = gpu.render_deep_view(orbit, view, mrd, palette=pal, supersample=s, bla=bla)
    everything = np.ones((view.height, view.width), bool)
    for window in TINY_WINDOWS:
        c0, r0, nc, nr = window
        img, st = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=0, window=window, bla=bla)
        assert np.array_equal(img, full[r0:r0 + nr, c0:c0 + nc]), window
        assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, everything, bla, window), window


def test_both_tables_of_a_render_stay_resident_and_a_third_span_takes_only_one_place(gpu):
    """Three dcmax in turn on one orbit (the two of an adaptive render, then a plain launch's, then the two again) and another
    orbit's render in between: every result is its model's, and the first render comes back bit for bit."""
    first, second = ("i-30-two-tables", 2), ("i-200-two-tables", 3)
    got = []
    for name, s in (first, second, (None, 0), first):
        if name is None:
            orbit, _, mrd, _, _ = K.case(first[0])
            third = DeepView(1e-12, 48, 40, 1e-12 * 40 / 48)
            zr, zi = orbit.table()
            mc, _, _ = B.counts(zr, zi, *D.offsets(third), mrd, B.build(zr, zi, B.dcmax(third)))
            c, _, _, _ = gpu.compute_deep_view(orbit, third, mrd, want_bytes=False, bla=True)
            assert np.array_equal(c.ravel(), mc)
            continue
        orbit, view, mrd, pal, mid = K.case(name)
        assert B.dcmax(view) != B.dcmax(K.finer(view, s))
        img, mask, st = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid, want_mask=True,
                                                      bla=True)
        got.append((img, mask, (st.pixel_iterations, st.never_pixels)))
    for (img, mask, st), (name, s) in zip(got, (first, second, first)):
        want, want_mask = _model(gpu, name, s, K.case(name)[4], True)
        assert np.array_equal(img, want) and np.array_equal(mask, want_mask), name
        assert st == _stats_model(gpu, name, s, want_mask, True), name
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1]) and got[0][2] == got[2][2]


@pytest.mark.parametrize("bla", [False, True], ids=["plain", "bla"])
def test_launch_on_a_torch_buffer_and_stream_equals_the_compute_form(gpu, bla):
    import torch
    orbit, view, mrd, pal, mid = K.case("i-30-two-tables")
    guard = 4096
    stream = torch.cuda.Stream()
    for s, window in [(2, None), (4, (19, 15, 22, 14))]:      # (the window holds the centre pixel and the edges around it)
        want, want_mask, _ = gpu.render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid, window=window,
                                                           want_mask=True, bla=bla)
        assert 0 < int(want_mask.sum()) < want_mask.size
        n, m = want.size, want_mask.size
        for with_mask in (True, False):
            buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            mbuf = torch.full((guard + m + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                gpu.launch_render_deep_view_adaptive(orbit, view, mrd, palette=pal, supersample=s, threshold=mid,
                                                     d_rgba=buf.data_ptr() + guard,
                                                     d_mask=mbuf.data_ptr() + guard if with_mask else 0,
                                                     stream=stream.cuda_stream, window=window, max_band_rows=7, bla=bla)
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
    orbit = K.orbit(("0", "1"), mrd, 1e-30)
    view = DeepView(1e-30, 64, 48, 1e-30 * 48 / 64)
    pal2 = np.zeros((2, 4), np.uint8)
    pal256 = np.zeros((256, 4), np.uint8)
    out = np.full((48, 64, 4), 0xA5, np.uint8)
    mask = np.full((48, 64), 0xA5, np.uint8)

    def spec(source=L.MBK_RENDER_SMOOTH, s=2, pal=pal2, scale=1.0):
        return L.mbk_render_spec(source, s, pal.ctypes.data if pal is not None else None, 2 if pal is None else len(pal),
                                 (C.c_uint8 * 4)(0, 0, 0, 255), scale, 0.0, 0)

    def call(sp, thr=17, cv=False, mrd=mrd, flags=0, dst=out, orb=orbit._h):
        cv = gpu._cdeep(view, None) if cv is False else cv
        st = lib.mbk_deep_view_render_adaptive_compute(gpu._h, orb, C.byref(cv) if cv is not None else None, mrd, flags,
                                                       C.byref(sp) if sp is not None else None, thr,
                                                       dst.ctypes.data if dst is not None else None, mask.ctypes.data, None)
        assert (out == 0xA5).all() and (mask == 0xA5).all()
        return st

    big = DeepView(1e-30, 2 ** 29, 48, 1e-30)
    cases = {
        "threshold 257": lambda: call(spec(), thr=257),
        "threshold 2^32 - 1": lambda: call(spec(), thr=2 ** 32 - 1),
        "bytes": lambda: call(spec(source=L.MBK_RENDER_BYTES, pal=pal256)),
        "equalized": lambda: call(spec(source=L.MBK_RENDER_EQUALIZED)),
        "distance_rel": lambda: call(spec(source=L.MBK_RENDER_DISTANCE_REL)),
        "distance": lambda: call(spec(source=L.MBK_RENDER_DISTANCE)),
        "MBK_DEEP_XBLA": lambda: call(spec(), flags=L.MBK_DEEP_XBLA),
        "MBK_DEEP_XBLA beside MBK_DEEP_BLA": lambda: call(spec(), flags=L.MBK_DEEP_XBLA | L.MBK_DEEP_BLA),
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
        "W s overflows": lambda: call(spec(s=8), cv=gpu._cdeep(big, (0, 0, 64, 48))),
    }
    for name, case in cases.items():
        assert case() == L.MBK_ERR_INVALID, name
    assert call(spec(), flags=L.MBK_DEEP_XBLA) == L.MBK_ERR_INVALID and b"MBK_DEEP_XBLA" in lib.mbk_last_error(gpu._h)
    with pytest.raises(MbkError):
        gpu.render_deep_view_adaptive(orbit, view, mrd, palette=K.PAL, supersample=2, threshold=257)
    with pytest.raises(ValueError):
        gpu.render_deep_view_adaptive(orbit, WideDeepView(1.0, -100, 64, 48), mrd, palette=K.PAL, supersample=2, threshold=17)
    with pytest.raises(ValueError):
        gpu.launch_render_deep_view_adaptive(orbit, WideDeepView(1.0, -100, 64, 48), mrd, palette=K.PAL, supersample=2, threshold=17,
                                             d_rgba=out.ctypes.data)

    # the launch form refuses the same way: device buffers stay as they were
    import torch
    buf = torch.full((48 * 64 * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
    mbuf = torch.full((48 * 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cv = gpu._cdeep(view, None)
    for sp, thr, flags in ((spec(), 257, 0), (spec(source=L.MBK_RENDER_BYTES, pal=pal256), 17, 0), (spec(), 17, L.MBK_DEEP_XBLA),
                           (spec(), 17, L.MBK_KERNEL_ASM)):
        assert lib.mbk_deep_view_render_adaptive_launch(gpu._h, orbit._h, C.byref(cv), mrd, flags, C.byref(sp), thr, buf.data_ptr(),
                                                        mbuf.data_ptr(), None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_render_adaptive_launch(gpu._h, orbit._h, C.byref(cv), mrd, 0, C.byref(spec()), 17, None,
                                                    mbuf.data_ptr(), None) == L.MBK_ERR_INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all() and (mbuf.cpu().numpy() == 0x5A).all()
    # and a good call works afterwards
    ok = np.empty((48, 64, 4), np.uint8)
    for flags in (0, L.MBK_DEEP_BLA):
        assert lib.mbk_deep_view_render_adaptive_compute(gpu._h, orbit._h, C.byref(cv), mrd, flags, C.byref(spec()), 17,
                                                         ok.ctypes.data, None, None) == L.MBK_OK
