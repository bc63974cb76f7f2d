"""Rendering on the GPU (include/mbk.h, "Rendering"): the image a render returns is held bit for bit to the numpy restatement
of the contract (tests/render_model.py) applied to the samples the same device returns for the finer view, through every entry
point; the Viewer palette is pinned to the reference Viewer's recorded output on whole DataChunks."""
import ctypes as C
import os

import numpy as np
import pytest

import render_model as M
from conftest import ROOT
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import datachunk_geometry

pytestmark = pytest.mark.gpu

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")
PLAIN = {   # name: (centre_r, centre_i, span, mrd)
    "full-set": (-0.5, 0.0, 3.0, 300),
    "inset-boundary": (-0.1, 0.65, 0.2, 400),          # the top of the main cardioid: interior, boundary and exterior
    "cfg3-centre": (-0.743643, 0.131825, 1e-5, 1500),
}
DEEP = {    # name: (centre, span, mrd)
    "seahorse-1e-20": (SEAHORSE, 1e-20, 30000),
    "i-1e-60": (("0", "1"), 1e-60, 5000),              # below the 1e-13 span binary64 views stop at
}
SMOOTH_PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255))    # neither length nor scale is a power of two
RANDOM_PAL = Palette(np.random.RandomState(1).randint(0, 256, (256, 4)).astype(np.uint8))


def _size(s):
    """Output sizes that are multiples neither of 8 nor of any s; smaller where s^2 samples per pixel make the model slow."""
    return (509, 383) if s <= 3 else (253, 189)


def _model_smooth(pal, s, counts, nu):
    out = [M.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, s, counts[r:r + 64 * s], nu[r:r + 64 * s])
           for r in range(0, counts.shape[0], 64 * s)]
    return np.concatenate(out)


def _plain_view(name, s, mult=1):
    cr, ci, span, mrd = PLAIN[name]
    w, h = _size(s)
    return View(cr - span / 2, ci - span / 2 * h / w, span, span * h / w, w * mult, h * mult), mrd


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


def _finer_deep(view, s):
    return DeepView(view.span_r, view.width * s, view.height * s, view.span_i)


@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_views_equal_the_model_on_the_devices_own_samples(gpu, name, s):
    view, mrd = _plain_view(name, s)
    nu, counts, st_s = gpu.compute_view_smooth(_finer(view, s), mrd)
    _, byts, _ = gpu.compute_view(_finer(view, s), mrd, want_counts=False)
    assert len(np.unique(counts)) > 10
    img, st = gpu.render_view(view, mrd, palette=SMOOTH_PAL, source="smooth", supersample=s)
    assert img.shape == (view.height, view.width, 4) and img.dtype == np.uint8
    want = _model_smooth(SMOOTH_PAL, s, counts, nu)
    assert np.array_equal(img, want), int((img != want).any(axis=2).sum())
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    assert st.kernel_ms > 0 and not st.all_bytes_zero and not st.all_bytes_one and st.rle_runs == 0
    for pal in (Palette.viewer(), RANDOM_PAL):
        img, st = gpu.render_view(view, mrd, palette=pal, source="bytes", supersample=s)
        want = M.render_bytes(pal.entries, s, byts)
        assert np.array_equal(img, want), int((img != want).any(axis=2).sum())
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)


@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("name", list(DEEP))
def test_deep_views_equal_the_model_on_the_devices_own_samples(gpu, name, s):
    centre, span, mrd = DEEP[name]
    orbit = DeepOrbit(*centre, mrd, min_span=span)
    view = DeepView(span, *_size(s))
    counts, byts, nu, st_s = gpu.compute_deep_view(orbit, _finer_deep(view, s), mrd, want_smooth=True)
    assert len(np.unique(counts)) > 10
    img, st = gpu.render_deep_view(orbit, view, mrd, palette=SMOOTH_PAL, source="smooth", supersample=s)
    want = _model_smooth(SMOOTH_PAL, s, counts, nu)
    assert np.array_equal(img, want), int((img != want).any(axis=2).sum())
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    img, st = gpu.render_deep_view(orbit, view, mrd, palette=RANDOM_PAL, source="bytes", supersample=s)
    want = M.render_bytes(RANDOM_PAL.entries, s, byts)
    assert np.array_equal(img, want), int((img != want).any(axis=2).sum())
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)


@pytest.mark.parametrize("level, mrd, ir, ii", [(4, 256, 1, 2), (8, 256, 2, 4)])
def test_viewer_palette_on_a_datachunk_is_what_the_reference_viewer_shows(gpu, level, mrd, ir, ii):
    """All 4096^2 pixels: the render of a DataChunk's view through Palette.viewer() equals the 8-bit form of the reference
    Viewer's data_to_img_array (tests/golden/viewer_palette.npz) applied to the chunk the worker path produces."""
    table = np.load(os.path.join(ROOT, "tests", "golden", "viewer_palette.npz"))["rgba8"]
    sr, si, rng = datachunk_geometry(level, ir, ii)
    byts, _, st = gpu.datachunk(level, mrd, ir, ii)
    assert not st.all_bytes_zero and not st.all_bytes_one and len(np.unique(byts)) > 20
    img, _ = gpu.render_view(View(sr, si, rng, rng, 4096, 4096), mrd, palette=Palette.viewer(), source="bytes")
    assert np.array_equal(img, table[byts].reshape(4096, 4096, 4))
    # a render leaves mbk_serialize_last on the last tile with bytes
    stream, _ = gpu.serialize_last()
    assert len(stream) > 1


def test_windows_and_band_heights_do_not_change_the_image(gpu):
    view, mrd = _plain_view("full-set", 2)
    orbit = DeepOrbit("1e-21", "1", 5000, min_span=1e-20)
    dview = DeepView(1e-20, 203, 131)
    for s, source, pal in [(2, "smooth", SMOOTH_PAL), (3, "bytes", RANDOM_PAL)]:
        whole, _ = gpu.render_view(view, mrd, palette=pal, source=source, supersample=s)
        dwhole, _ = gpu.render_deep_view(orbit, dview, 5000, palette=pal, source=source, supersample=s)
        assert len(np.unique(whole.reshape(-1, 4), axis=0)) > 50 and len(np.unique(dwhole.reshape(-1, 4), axis=0)) > 5
        for rows in (1, 7, 64, 0):
            img, _ = gpu.render_view(view, mrd, palette=pal, source=source, supersample=s, max_band_rows=rows)
            assert np.array_equal(img, whole), (source, rows)
            img, _ = gpu.render_deep_view(orbit, dview, 5000, palette=pal, source=source, supersample=s, max_band_rows=rows)
            assert np.array_equal(img, dwhole), (source, rows)
        for window in [(0, 40, view.width, 33), (13, 0, 101, view.height), (view.width - 1, view.height - 1, 1, 1),
                       (64, 64, 9, 8), (3, 5, 258, 70)]:
            c0, r0, nc, nr = window
            img, _ = gpu.render_view(view, mrd, palette=pal, source=source, supersample=s, window=window, max_band_rows=16)
            assert np.array_equal(img, whole[r0:r0 + nr, c0:c0 + nc]), (source, window)
        c0, r0, nc, nr = 17, 9, 150, 77
        img, _ = gpu.render_deep_view(orbit, dview, 5000, palette=pal, source=source, supersample=s, window=(c0, r0, nc, nr))
        assert np.array_equal(img, dwhole[r0:r0 + nr, c0:c0 + nc]), source


def test_a_render_of_two_bands_under_the_default_budget_equals_the_model(gpu):
    s, w, h, mrd = 8, 601, 590, 64
    assert w * h * s * s * 12 > L.MBK_RENDER_BAND_BYTES > w * h * s * s * 12 // 2
    view = View(-2.0, -1.25, 2.5 * w / h, 2.5, w, h)
    img, st = gpu.render_view(view, mrd, palette=SMOOTH_PAL, supersample=s)
    nu, counts, st_s = gpu.compute_view_smooth(_finer(view, s), mrd)
    assert np.array_equal(img, _model_smooth(SMOOTH_PAL, s, counts, nu))
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)


def test_launch_on_a_torch_buffer_and_stream_equals_render_view(gpu):
    import torch
    view, mrd = _plain_view("inset-boundary", 2)
    orbit = DeepOrbit("0", "1", 5000, min_span=1e-60)
    dview = DeepView(1e-60, 150, 131)
    guard = 4096
    stream = torch.cuda.Stream()
    for s, source, pal in [(2, "smooth", SMOOTH_PAL), (4, "bytes", Palette.viewer()), (1, "bytes", RANDOM_PAL)]:
        for window in (None, (7, 11, 301, 202)):
            want, _ = gpu.render_view(view, mrd, palette=pal, source=source, supersample=s, window=window)
            n = want.size
            buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                gpu.launch_render_view(view, mrd, palette=pal, d_rgba=buf.data_ptr() + guard, source=source, supersample=s,
                                       stream=stream.cuda_stream, window=window, max_band_rows=50)
            stream.synchronize()
            got = buf.cpu().numpy()
            assert np.array_equal(got[guard:guard + n].reshape(want.shape), want), (source, window)
            assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all(), (source, window)
        want, _ = gpu.render_deep_view(orbit, dview, 5000, palette=pal, source=source, supersample=s)
        buf = torch.full((guard + want.size + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            gpu.launch_render_deep_view(orbit, dview, 5000, palette=pal, d_rgba=buf.data_ptr() + guard, source=source,
                                        supersample=s, stream=stream.cuda_stream)
        stream.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[guard:guard + want.size].reshape(want.shape), want), source
        assert (got[:guard] == 0xA5).all() and (got[guard + want.size:] == 0xA5).all(), source


def test_every_kernel_selector_gives_the_same_image(gpu):
    # large enough for the default to take the scan / group decision from the window (>= 16384 blocks of 8 x 8 samples)
    view = View(-2.0, -1.5, 3.0, 3.0, 521, 517)
    mrd = 300
    want, _ = gpu.render_view(view, mrd, palette=SMOOTH_PAL, supersample=2)
    for kernel in ("asm", "group", "scan"):
        img, _ = gpu.render_view(view, mrd, palette=SMOOTH_PAL, supersample=2, kernel=kernel)
        assert np.array_equal(img, want), kernel
    want, _ = gpu.render_view(view, mrd, palette=RANDOM_PAL, source="bytes", supersample=2)
    for kernel in ("simple", "asm", "refill", "group", "scan"):
        img, _ = gpu.render_view(view, mrd, palette=RANDOM_PAL, source="bytes", supersample=2, kernel=kernel)
        assert np.array_equal(img, want), kernel


def test_palette_sizes_either_side_of_the_lds_limit(gpu):
    """Palettes of 16384 entries are staged in LDS, longer ones are read through the caches: same image as the model."""
    view, mrd = _plain_view("full-set", 4)
    nu, counts, _ = gpu.compute_view_smooth(_finer(view, 2), mrd)
    rs = np.random.RandomState(3)
    for n in (2, 16384, 16385, 65536):
        pal = Palette(rs.randint(0, 256, (n, 4)).astype(np.uint8), inside=(1, 2, 3, 4), scale=n / 9.7, offset=0.25)
        img, _ = gpu.render_view(view, mrd, palette=pal, supersample=2)
        assert np.array_equal(img, _model_smooth(pal, 2, counts, nu)), n


def test_refusals_leave_the_output_untouched(gpu):
    lib = L.load()
    view = View(-2.0, -1.5, 3.0, 3.0, 64, 48)
    orbit = DeepOrbit("0", "1", 500, min_span=1e-20)
    pal256 = np.zeros((256, 4), np.uint8)
    pal2 = np.zeros((2, 4), np.uint8)

    def spec(source=L.MBK_RENDER_BYTES, s=1, pal=pal256, n=None, scale=1.0, offset=0.0):
        return L.mbk_render_spec(source, s, pal.ctypes.data if pal is not None else None, len(pal) if n is None else n,
                                 (C.c_uint8 * 4)(0, 0, 0, 255), scale, offset, 0)

    def cview(v=view, window=None):
        return gpu._cview(v, window)

    out = np.full((48, 64, 4), 0xA5, np.uint8)

    def plain(sp, cv=None, mrd=256, flags=0, dst=out):
        cv = cview() if cv is None else cv
        st = lib.mbk_view_render_compute(gpu._h, C.byref(cv), mrd, flags, C.byref(sp) if sp is not None else None,
                                         dst.ctypes.data if dst is not None else None, None)
        assert (out == 0xA5).all()
        return st

    sm = dict(source=L.MBK_RENDER_SMOOTH, pal=pal2)
    cases = {
        "NULL spec": lambda: plain(None),
        "NULL palette": lambda: plain(spec(pal=None, n=256)),
        "NULL output": lambda: plain(spec(), dst=None),
        "unknown source": lambda: plain(spec(source=2)),
        "s = 5": lambda: plain(spec(s=5)), "s = 0": lambda: plain(spec(s=0)),
        "bytes palette of 2": lambda: plain(spec(pal=pal2)),
        "smooth palette of 1": lambda: plain(spec(source=L.MBK_RENDER_SMOOTH, pal=pal2, n=1)),
        "smooth palette of 65537": lambda: plain(spec(source=L.MBK_RENDER_SMOOTH, pal=np.zeros((65537, 4), np.uint8))),
        "scale 0": lambda: plain(spec(scale=0.0, **sm)), "scale nan": lambda: plain(spec(scale=np.nan, **sm)),
        "scale > 2^20": lambda: plain(spec(scale=2.0 ** 21, **sm)),
        "offset inf": lambda: plain(spec(offset=np.inf, **sm)), "offset < -2^20": lambda: plain(spec(offset=-2.0 ** 21, **sm)),
        "W s overflows": lambda: plain(spec(s=8), cv=cview(View(-2.0, -1.5, 3.0, 3.0, 2 ** 29, 48), (0, 0, 64, 48))),
        "sample window > 2^31": lambda: plain(spec(s=8), cv=cview(View(-2.0, -1.5, 3.0, 3.0, 2 ** 16, 2 ** 16), (0, 0, 2 ** 15, 2 ** 13))),
        "window exceeds the view": lambda: plain(spec(), cv=cview(window=(1, 0, 64, 48))),
        "empty window": lambda: plain(spec(), cv=cview(window=(0, 0, 0, 48))),
        "view not finite": lambda: plain(spec(), cv=cview(View(np.nan, -1.5, 3.0, 3.0, 64, 48))),
        "mrd 0 with bytes": lambda: plain(spec(), mrd=0),
        "mrd 2^31": lambda: plain(spec(), mrd=2 ** 31),
        "smooth with simple": lambda: plain(spec(**sm), flags=L.MBK_KERNEL_SIMPLE),
        "smooth with refill": lambda: plain(spec(**sm), flags=L.MBK_KERNEL_REFILL),
        "smooth with fp32": lambda: plain(spec(**sm), flags=L.MBK_PRECISION_F32),
        "unknown kernel": lambda: plain(spec(), flags=0x700),
        "an output flag": lambda: plain(spec(), flags=L.MBK_WANT_COUNTS),
        "lazy uniform": lambda: plain(spec(), flags=L.MBK_LAZY_UNIFORM),
    }
    for name, call in cases.items():
        assert call() == L.MBK_ERR_INVALID, name

    dv = gpu._cdeep(DeepView(1e-20, 64, 48), None)

    def deep(sp, orb=orbit, cv=dv, mrd=256, flags=0):
        st = lib.mbk_deep_view_render_compute(gpu._h, orb._h if orb is not None else None, C.byref(cv), mrd, flags,
                                              C.byref(sp), out.ctypes.data, None)
        assert (out == 0xA5).all()
        return st

    assert deep(spec(), orb=None) == L.MBK_ERR_INVALID
    assert deep(spec(), mrd=501) == L.MBK_ERR_INVALID                       # beyond the orbit's mrd
    assert deep(spec(), flags=L.MBK_KERNEL_GROUP) == L.MBK_ERR_INVALID      # deep renders take no flags
    assert deep(spec(s=5)) == L.MBK_ERR_INVALID
    assert deep(spec(), cv=gpu._cdeep(DeepView(8.0, 64, 48, 8.0), None)) == L.MBK_ERR_INVALID
    assert deep(spec(), mrd=0) == L.MBK_ERR_INVALID

    # the launch form refuses the same way: a device buffer stays as it was
    import torch
    buf = torch.full((48 * 64 * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cv = cview()
    for sp in (spec(s=5), spec(pal=pal2), spec(scale=0.0, **sm)):
        assert lib.mbk_view_render_launch(gpu._h, C.byref(cv), 256, 0, C.byref(sp), buf.data_ptr(), None) == L.MBK_ERR_INVALID
    assert lib.mbk_view_render_launch(gpu._h, C.byref(cv), 256, 0, C.byref(spec()), None, None) == L.MBK_ERR_INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all()

    # slot 0 busy: the synchronous renders are refused, and work again after the wait
    tile = gpu.pinned_empty((L.MBK_CHUNK_BYTES,), np.uint8)
    gpu.submit_datachunk(0, 4, 256, 1, 2, tile)
    assert plain(spec()) == L.MBK_ERR_INVALID
    assert deep(spec()) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.render_view(view, 256, palette=Palette.viewer(), source="bytes")
    gpu.wait(0)
    ok = np.empty((48, 64, 4), np.uint8)
    assert lib.mbk_view_render_compute(gpu._h, C.byref(cview()), 256, 0, C.byref(spec()), ok.ctypes.data, None) == L.MBK_OK
    assert (out == 0xA5).all()
