"""Adaptive supersampling on the GPU (include/mbk.h, "Adaptive supersampling"): image and mask are held bit for bit to the numpy
restatement of the contract (tests/adaptive_model.py) applied to the samples the same device returns for the view and for the
s times finer view, as tests/test_gpu_render.py holds the plain renders; thresholds 0 and 256 also to render_view itself."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as A
import render_model as M
from distributedmandelbrot_amd import MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L

pytestmark = pytest.mark.gpu

# Multiples neither of 8 nor of any s; 3015 pixels: at s = 2 a full list is 189 groups of 16, the last one part-filled.
W, H = 67, 45
# name: (centre_r, centre_i, span, mrd, middle threshold).  The views are test_gpu_render.py's.  The middle thresholds were read
# off a plain numpy iteration of the two views at 67 x 45 under PAL (refined shares 0.24 and 0.34); the tests assert 5 % .. 60 %
# on the model's mask of the device's samples.
VIEWS = {
    "inset-boundary": (-0.1, 0.65, 0.2, 400, 32),
    "cfg3-centre": (-0.743643, 0.131825, 1e-5, 1500, 245),
}
PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255))    # test_gpu_render.py's SMOOTH_PAL
_cache = {}


def _view(name):
    cr, ci, span, mrd, thr = VIEWS[name]
    return View(cr - span / 2, ci - span / 2 * H / W, span, span * H / W, W, H), mrd, thr


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


def _samples(gpu, name, s):
    """(nu, counts) of the view at s times the resolution, from the device; computed once per (view, s) and left unchanged."""
    if (name, s) not in _cache:
        view, mrd, _ = _view(name)
        nu, counts, _ = gpu.compute_view_smooth(_finer(view, s), mrd)
        nu.setflags(write=False)
        counts.setflags(write=False)
        _cache[name, s] = (nu, counts)
    return _cache[name, s]


def _model(gpu, name, s, thr, pal=PAL):
    bn, bc = _samples(gpu, name, 1)
    fn, fc = _samples(gpu, name, s)
    return A.render_adaptive(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, bc, bn, fc, fn)


def _stats_model(gpu, name, s, mask, window=None):
    _, mrd, _ = _view(name)
    return A.sample_stats(mask, mrd, s, _samples(gpu, name, 1)[1], _samples(gpu, name, s)[1], window)


@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("name", list(VIEWS))
def test_image_mask_and_statistics_equal_the_model_on_the_devices_own_samples(gpu, name, s):
    view, mrd, mid = _view(name)
    for thr in (0, mid, 256):
        want, want_mask = _model(gpu, name, s, thr)
        share = want_mask.mean()
        print(name, s, thr, "refined share of the model's mask:", share)
        if thr == mid:
            assert 0.05 <= share <= 0.60, share      # neither an empty nor a full list
        img, mask, st = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=thr, want_mask=True)
        assert img.shape == (H, W, 4) and img.dtype == np.uint8 and mask.shape == (H, W) and mask.dtype == np.uint8
        assert np.array_equal(mask, want_mask), (thr, int((mask != want_mask).sum()))
        assert np.array_equal(img, want), (thr, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, want_mask), thr
        assert st.kernel_ms > 0 and not st.all_bytes_zero and not st.all_bytes_one and st.rle_runs == 0
        # without a mask: the same image
        img2, _ = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=thr)
        assert np.array_equal(img2, img), thr
        if thr == 0:
            full, _ = gpu.render_view(view, mrd, palette=PAL, supersample=s)
            assert mask.all() and np.array_equal(img, full)
        if thr == 256:
            one, _ = gpu.render_view(view, mrd, palette=PAL, supersample=1)
            assert not mask.any() and np.array_equal(img, one)


@pytest.mark.parametrize("kernel", ["asm", "group", "scan"])
def test_every_kernel_selector_gives_the_same_image(gpu, kernel):
    """asm also runs the refine kernel on the per-step loop instead of the grouped loop with the cycle test."""
    name, s = "inset-boundary", 3
    view, mrd, mid = _view(name)
    want, want_mask = _model(gpu, name, s, mid)
    img, mask, st = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=mid, kernel=kernel, want_mask=True)
    assert np.array_equal(img, want) and np.array_equal(mask, want_mask)
    assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, want_mask)


# odd offsets, touching the right and the top edge of the view; touching no edge
WINDOWS = [(45, 31, 22, 14), (3, 5, 31, 17)]


@pytest.mark.parametrize("name", list(VIEWS))
def test_windows_and_bands_equal_the_same_rectangle_of_the_whole_image(gpu, name):
    s = 3
    view, mrd, mid = _view(name)
    whole, whole_mask = _model(gpu, name, s, mid)
    for window in WINDOWS:
        c0, r0, nc, nr = window
        for rows in (0, 4):
            img, mask, st = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=mid, window=window,
                                                     max_band_rows=rows, want_mask=True)
            assert np.array_equal(img, whole[r0:r0 + nr, c0:c0 + nc]), (window, rows)
            assert np.array_equal(mask, whole_mask[r0:r0 + nr, c0:c0 + nc]), (window, rows)
            # the halo is not counted, and nothing twice across bands
            assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, whole_mask, window), (window, rows)
    # the halo crosses bands: band heights of 1 and 5 give the unbanded image
    for s in (2, 8):
        whole, whole_mask = _model(gpu, name, s, mid)
        for rows in (1, 5):
            img, mask, st = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=mid, max_band_rows=rows,
                                                     want_mask=True)
            assert np.array_equal(img, whole) and np.array_equal(mask, whole_mask), (s, rows)
            assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, whole_mask), (s, rows)


# One listed pixel is a list shorter than one group of the refine kernel's walk at s = 2, 3, 4 (16, 7, 4 pixels to a group) and
# three end inside a group; at s = 8 a pixel is a group.  Inside the view; touching its right and its bottom edge.
TINY_WINDOWS = [(33, 22, 1, 1), (W - 3, H - 1, 3, 1)]


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_lists_shorter_than_a_group_equal_the_same_pixels_of_the_full_render(gpu, s):
    name = "inset-boundary"
    view, mrd, _ = _view(name)
    full, _ = gpu.render_view(view, mrd, palette=PAL, supersample=s)
    everything = np.ones((H, W), bool)
    for window in TINY_WINDOWS:
        c0, r0, nc, nr = window
        img, st = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=0, window=window)
        assert np.array_equal(img, full[r0:r0 + nr, c0:c0 + nc]), window
        assert (st.pixel_iterations, st.never_pixels) == _stats_model(gpu, name, s, everything, window), window


def test_a_view_inside_the_main_cardioid_refines_nothing(gpu):
    view, mrd = View(-0.25, -0.05 * H / W, 0.1, 0.1 * H / W, W, H), 200
    for s in (2, 8):
        img, mask, st = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=1, want_mask=True)
        assert not mask.any()
        assert (img == np.array(PAL.inside, np.uint8)).all()
        assert (st.pixel_iterations, st.never_pixels) == (W * H * (mrd - 1), W * H)


@pytest.mark.parametrize("s", [2, 3, 4, 8])
def test_the_doubling_and_ring_rules_of_the_refine_kernel_against_the_existing_render(gpu, s):
    """Threshold 0: every pixel goes through the refine kernel, and the image is render_view's at s.  The first view straddles
    the real axis with a fine imaginary axis of non-zero |c_i| below 2^-900 (the literal doubling); the second holds
    c = -2 exactly, on the ring |c| = 2 (the per-step test)."""
    u = 2.0 ** -950
    tiny = View(-2.2, -3 * u, 2.8, 20 * u, W, H)
    ys = np.abs(np.linspace(tiny.start_i, tiny.start_i + tiny.range_i, H * s))
    assert ((ys != 0.0) & (ys < 2.0 ** -900)).any()
    ring = View(-2.0, 0.0, 1.0, 0.7, W, H)
    assert np.linspace(-2.0, -1.0, W * s)[0] == -2.0 and np.linspace(0.0, 0.7, H * s)[0] == 0.0
    for view, mrd in ((tiny, 300), (ring, 300)):
        want, _ = gpu.render_view(view, mrd, palette=PAL, supersample=s)
        assert len(np.unique(want.reshape(-1, 4), axis=0)) > 10
        for kernel in ("default", "asm"):
            img, mask, _ = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=0, kernel=kernel,
                                                    want_mask=True)
            assert mask.all() and np.array_equal(img, want), (kernel, int((img != want).any(axis=2).sum()))


def test_launch_on_a_torch_buffer_and_stream_equals_the_compute_form(gpu):
    import torch
    name = "inset-boundary"
    view, mrd, mid = _view(name)
    guard = 4096
    stream = torch.cuda.Stream()
    for s, window in [(2, None), (4, (45, 31, 22, 14))]:
        want, want_mask, _ = gpu.render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=mid, window=window,
                                                      want_mask=True)
        n, m = want.size, want_mask.size
        for with_mask in (True, False):
            buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            mbuf = torch.full((guard + m + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                gpu.launch_render_view_adaptive(view, mrd, palette=PAL, supersample=s, threshold=mid, d_rgba=buf.data_ptr() + guard,
                                                d_mask=mbuf.data_ptr() + guard if with_mask else 0,
                                                stream=stream.cuda_stream, window=window, max_band_rows=7)
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
    view = View(-2.0, -1.5, 3.0, 3.0, 64, 48)
    pal2 = np.zeros((2, 4), np.uint8)
    pal256 = np.zeros((256, 4), np.uint8)
    out = np.full((48, 64, 4), 0xA5, np.uint8)
    mask = np.full((48, 64), 0xA5, np.uint8)

    def spec(source=L.MBK_RENDER_SMOOTH, s=2, pal=pal2, scale=1.0):
        return L.mbk_render_spec(source, s, pal.ctypes.data if pal is not None else None, 2 if pal is None else len(pal),
                                 (C.c_uint8 * 4)(0, 0, 0, 255), scale, 0.0, 0)

    def call(sp, thr=17, cv=None, mrd=256, flags=0, dst=out):
        cv = gpu._cview(view, None) if cv is None else cv
        st = lib.mbk_view_render_adaptive_compute(gpu._h, C.byref(cv), mrd, flags, C.byref(sp) if sp is not None else None, thr,
                                                  dst.ctypes.data if dst is not None else None, mask.ctypes.data, None)
        assert (out == 0xA5).all() and (mask == 0xA5).all()
        return st

    cases = {
        "threshold 257": lambda: call(spec(), thr=257),
        "threshold 2^32 - 1": lambda: call(spec(), thr=2 ** 32 - 1),
        "bytes": lambda: call(spec(source=L.MBK_RENDER_BYTES, pal=pal256)),
        "distance": lambda: call(spec(source=L.MBK_RENDER_DISTANCE)),
        "equalized": lambda: call(spec(source=L.MBK_RENDER_EQUALIZED)),
        "unknown source": lambda: call(spec(source=2)),
        "fp32": lambda: call(spec(), flags=L.MBK_PRECISION_F32),
        "simple": lambda: call(spec(), flags=L.MBK_KERNEL_SIMPLE),
        "refill": lambda: call(spec(), flags=L.MBK_KERNEL_REFILL),
        "an output flag": lambda: call(spec(), flags=L.MBK_WANT_COUNTS),
        "NULL spec": lambda: call(None),
        "NULL palette": lambda: call(spec(pal=None)),
        "NULL output": lambda: call(spec(), dst=None),
        "s = 5": lambda: call(spec(s=5)),
        "scale 0": lambda: call(spec(scale=0.0)),
        "mrd 2^31": lambda: call(spec(), mrd=2 ** 31),
        "window exceeds the view": lambda: call(spec(), cv=gpu._cview(view, (1, 0, 64, 48))),
        "empty window": lambda: call(spec(), cv=gpu._cview(view, (0, 0, 0, 48))),
        "W s overflows": lambda: call(spec(s=8), cv=gpu._cview(View(-2.0, -1.5, 3.0, 3.0, 2 ** 29, 48), (0, 0, 64, 48))),
    }
    for name, case in cases.items():
        assert case() == L.MBK_ERR_INVALID, name
    with pytest.raises(MbkError):
        gpu.render_view_adaptive(view, 256, palette=PAL, supersample=2, threshold=257)

    # the launch form refuses the same way: device buffers stay as they were
    import torch
    buf = torch.full((48 * 64 * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
    mbuf = torch.full((48 * 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cv = gpu._cview(view, None)
    for sp, thr, flags in ((spec(), 257, 0), (spec(source=L.MBK_RENDER_BYTES, pal=pal256), 17, 0), (spec(), 17, L.MBK_PRECISION_F32)):
        assert lib.mbk_view_render_adaptive_launch(gpu._h, C.byref(cv), 256, flags, C.byref(sp), thr, buf.data_ptr(),
                                                   mbuf.data_ptr(), None) == L.MBK_ERR_INVALID
    assert lib.mbk_view_render_adaptive_launch(gpu._h, C.byref(cv), 256, 0, C.byref(spec()), 17, None, mbuf.data_ptr(),
                                               None) == L.MBK_ERR_INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all() and (mbuf.cpu().numpy() == 0x5A).all()
    # and a good call works afterwards
    ok = np.empty((48, 64, 4), np.uint8)
    assert lib.mbk_view_render_adaptive_compute(gpu._h, C.byref(cv), 256, 0, C.byref(spec()), 17, ok.ctypes.data, None,
                                                None) == L.MBK_OK
