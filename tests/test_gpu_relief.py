"""Relief shading on the GPU (include/mbk.h, "Relief shading"), held to the numpy model of the contract (tests/relief_model.py).

The normals involve no libm call, so the device must store the model's value on every pixel and bit, with every kernel
selector: "asm" is the one-pass form, the others the two-pass form.  The counts are compute_view's, the optional distance
estimates compute_view_distance's bits.  A relief render is mbk_relief_resolve_host (held to the numpy rule by
tests/test_relief.py) of the device's own smooth samples and normals of the s times finer view, banded or not, whole or windowed.
The shapes are the smallest at which the kernels can go wrong: ragged against the 8x8 blocks, more than one block, whole-interior
blocks, a single row.
"""
import ctypes as C
import math

import numpy as np
import pytest

import relief_model as RM
from distributedmandelbrot_amd import MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import relief_resolve_host

pytestmark = pytest.mark.gpu

KERNELS = ["default", "scan", "group", "asm"]
SEAHORSE = ((-0.765, 0.085, 0.04, 0.04 * 44 / 66, 67, 45), 600)      # neither side a multiple of 8
_MODEL = {}


def _model(v, mrd, window=None):
    key = (v, mrd, window)
    if key not in _MODEL:
        _MODEL[key] = RM.model(v, mrd, window)
    return _MODEL[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("kernel", KERNELS)
def test_normals_equal_the_model_on_every_pixel_and_bit(gpu, kernel):
    v, mrd = SEAHORSE
    view = View(*v)
    want, mn, _ = _model(v, mrd)
    assert (mn == 0).sum() > 50 and len(np.unique(mn)) > 40 and (want[mn > 0] != 0.0).any(axis=1).all()
    ref, _, _ = gpu.compute_view(view, mrd, want_bytes=False)
    counts, normals, stats = gpu.compute_view_normals(view, mrd, kernel=kernel)
    assert counts.dtype == np.int32 and normals.dtype == np.float64 and normals.shape == (45, 67, 2)
    assert np.array_equal(counts, ref) and np.array_equal(counts, mn)
    assert _same_bits(normals, want), int((_bits(normals) != _bits(want)).any(axis=2).sum())
    assert not np.isnan(normals).any() and not normals[counts == 0].any()
    assert stats.pixel_iterations == int(np.where(counts > 0, counts, mrd - 1).astype(np.int64).sum())
    assert stats.never_pixels == int((counts == 0).sum())
    # with the distance estimates: the same normals, and the bits compute_view_distance stores
    de_ref, dc, _ = gpu.compute_view_distance(view, mrd, kernel=kernel)
    c2, n2, de, _ = gpu.compute_view_normals(view, mrd, kernel=kernel, want_distance=True)
    assert np.array_equal(c2, counts) and np.array_equal(dc, counts) and _same_bits(n2, want)
    assert _same_bits(de, de_ref) and (de[counts > 0] > 0.0).all()


@pytest.mark.parametrize("kernel", ["default", "asm"])
def test_window_equals_the_same_pixels_of_the_whole_view(gpu, kernel):
    view, mrd = View(-2.0, -1.25, 2.75, 2.5, 128, 96), 300
    wc, whole, _ = gpu.compute_view_normals(view, mrd, kernel=kernel)
    assert (wc == 0).any() and len(np.unique(wc)) > 20
    c0, r0, nc, nr = window = (5, 3, 21, 17)
    c, n, de, st = gpu.compute_view_normals(view, mrd, window=window, kernel=kernel, want_distance=True)
    assert np.array_equal(c, wc[r0:r0 + nr, c0:c0 + nc]) and _same_bits(n, whole[r0:r0 + nr, c0:c0 + nc])
    assert _same_bits(de, gpu.compute_view_distance(view, mrd, window=window, kernel=kernel)[0])
    assert st.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
    want, mn, _ = _model((-2.0, -1.25, 2.75, 2.5, 128, 96), mrd, window)
    assert np.array_equal(c, mn) and _same_bits(n, want)


def _device_buffers(torch, px, guard):
    dn = torch.full((2 * (px + 2 * guard),), -77.0, dtype=torch.float64, device="cuda:0")
    dd = torch.full((px + 2 * guard,), -78.0, dtype=torch.float64, device="cuda:0")
    dc = torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0")
    return dn, dd, dc


@pytest.mark.parametrize("kernel", KERNELS)
def test_launch_writes_every_element_zeros_included_and_nothing_else(gpu, kernel):
    """A 64 x 64 view that holds whole-interior 8x8 blocks (part of the main cardioid) and the edge: the launch form on a torch
    stream into buffers prefilled with a sentinel, guard rows in front of and behind the window."""
    import torch
    v, mrd = (-0.4, 0.2, 0.6, 0.6, 64, 64), 300
    view = View(*v)
    want, mn, _ = _model(v, mrd)
    blocks = (mn.reshape(8, 8, 8, 8) == 0).all(axis=(1, 3))
    assert blocks.sum() >= 8 and (mn > 0).sum() > 500 and not blocks.all()
    px, guard = 64 * 64, 3 * 64
    stream = torch.cuda.Stream(device="cuda:0")
    forms = [(True, True), (False, False), (True, False)]            # (with d_counts, with d_distance)
    bufs = [_device_buffers(torch, px, guard) for _ in forms]
    torch.cuda.synchronize()
    for (dn, dd, dc), (with_counts, with_de) in zip(bufs, forms):
        gpu.launch_view_normals(view, mrd, d_normals=dn[2 * guard:].data_ptr(), d_counts=dc[guard:].data_ptr() if with_counts else 0,
                                d_distance=dd[guard:].data_ptr() if with_de else 0, stream=stream.cuda_stream, kernel=kernel)
    stream.synchronize()
    de_ref = gpu.compute_view_distance(view, mrd, kernel=kernel)[0]
    for (dn, dd, dc), (with_counts, with_de) in zip(bufs, forms):
        hn, hd, hc = dn.cpu().numpy(), dd.cpu().numpy(), dc.cpu().numpy()
        got = hn[2 * guard:2 * (guard + px)].reshape(64, 64, 2)
        assert _same_bits(got, want), (with_counts, with_de)
        assert not got[mn == 0].any() and not np.signbit(got[mn == 0]).any()          # zeros, written
        assert (hn[:2 * guard] == -77.0).all() and (hn[2 * (guard + px):] == -77.0).all()
        assert (hd[:guard] == -78.0).all() and (hd[guard + px:] == -78.0).all()
        assert (hc[:guard] == -5).all() and (hc[guard + px:] == -5).all()
        assert np.array_equal(hc[guard:guard + px].reshape(64, 64), mn) if with_counts else (hc == -5).all()
        assert _same_bits(hd[guard:guard + px].reshape(64, 64), de_ref) if with_de else (hd == -78.0).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_degenerate_inputs(gpu, kernel):
    v = (-2.0, -2.0, 4.0, 4.0, 16, 16)
    for mrd in (0, 1, 2):
        c, n, de, st = gpu.compute_view_normals(View(*v), mrd, kernel=kernel, want_distance=True)
        want, mn, _ = _model(v, mrd)
        assert np.array_equal(c, mn) and _same_bits(n, want) and _same_bits(de, gpu.compute_view_distance(View(*v), mrd, kernel=kernel)[0])
        if mrd < 2:
            assert not c.any() and not n.any() and st.pixel_iterations == 0 and st.never_pixels == 256
        else:
            assert set(np.unique(c)) == {0, 1} and (n[c == 1] != 0.0).any(axis=1).all()
    # |c| ~ 1e80 at the corners: z_1 overflows mag, |z conj(d)|^2 overflows: count 1 and the flat normal; the centre pixel is c = 0
    big = (-1e80, -1e80, 2e80, 2e80, 9, 9)
    c, n, _ = gpu.compute_view_normals(View(*big), 50, kernel=kernel)
    want, mn, _ = _model(big, 50)
    assert np.array_equal(c, mn) and _same_bits(n, want)
    assert c[0, 0] == c[8, 8] == c[0, 8] == 1 and c[4, 4] == 0 and not n.any() and not np.isnan(n).any()
    # a pixel that is c = -2 exactly: z sits at 2 through the whole run-on, d stays finite: nx = -1
    line = (-2.0, 0.0, 1.0, 0.0, 5, 1)
    c, n, _ = gpu.compute_view_normals(View(*line), 100, kernel=kernel)
    want, mn, mst = _model(line, 100)
    assert np.array_equal(c, mn) and _same_bits(n, want)
    assert c[0, 0] == 1 and mst["extra"][0] == 64 and n[0, 0, 0] == -1.0 and n[0, 0, 1] == 0.0


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


RENDER_VIEW = ((-0.765, 0.085, 0.04, 0.04 * 27 / 39, 40, 28), 400)


def _render_palette():
    rng = np.random.RandomState(11)
    return Palette(rng.randint(0, 256, (53, 4)).astype(np.uint8), inside=(9, 8, 7, 200), scale=3.7, offset=0.25)


@pytest.mark.parametrize("kernel", ["default", "asm"])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_render_equals_the_host_rule_and_the_model(gpu, s, kernel):
    v, mrd = RENDER_VIEW
    view = View(*v)
    w, h = view.width, view.height
    pal = _render_palette()
    fine = _finer(view, s)
    nu, counts, st_s = gpu.compute_view_smooth(fine, mrd, kernel=kernel)
    c2, normals, _ = gpu.compute_view_normals(fine, mrd, kernel=kernel)
    mnorm, mn, _ = _model(v[:4] + (w * s, h * s), mrd)
    assert np.array_equal(counts, c2) and np.array_equal(counts, mn) and _same_bits(normals, mnorm)
    assert (counts == 0).any() and len(np.unique(counts)) > 10
    light, height = (math.cos(0.6), math.sin(0.6)), 1.25
    want = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=normals, light=light, height=height)
    model = RM.render(pal.entries, pal.inside, pal.scale, pal.offset, light[0], light[1], height, s, counts, nu, mnorm)
    assert np.array_equal(want, model) and len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    for rows in (0, 3):
        img, st = gpu.render_view_relief(view, mrd, palette=pal, light=light, height=height, supersample=s, kernel=kernel,
                                         max_band_rows=rows)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (7, 5, 19, 13)
    img, _ = gpu.render_view_relief(view, mrd, palette=pal, light=light, height=height, supersample=s, kernel=kernel, window=window)
    assert np.array_equal(img, want[5:18, 7:26])
    # the launch form on a caller's stream, guard words behind the image
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_view_relief(view, mrd, palette=pal, d_rgba=d.data_ptr(), light=light, height=height, supersample=s,
                                  kernel=kernel, stream=stream.cuda_stream, max_band_rows=5)
    stream.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


def test_render_lights_and_the_neutral_shade(gpu):
    v, mrd = RENDER_VIEW
    view = View(*v)
    pal = _render_palette()
    a, _ = gpu.render_view_relief(view, mrd, palette=pal)                                   # 45 degrees, height 1.5
    b, _ = gpu.render_view_relief(view, mrd, palette=pal, light_deg=200.0, height=0.5)
    lx, ly = float(np.cos(np.deg2rad(45.0))), float(np.sin(np.deg2rad(45.0)))
    assert np.array_equal(a, gpu.render_view_relief(view, mrd, palette=pal, light=(lx, ly), height=1.5)[0])
    assert (a != b).any(axis=2).sum() > 200
    # height 2^10 without a light: every escaped sample takes the neutral q = 255, the inside none
    flat, _ = gpu.render_view_relief(view, mrd, palette=pal, light=(0.0, 0.0), height=2.0 ** 10)
    smooth, _ = gpu.render_view(view, mrd, palette=pal, source="smooth")
    counts, _, _ = gpu.compute_view(view, mrd, want_bytes=False)
    assert RM.neutral(2.0 ** 10) == 255
    want = smooth.astype(np.int64)
    want[..., :3] = (want[..., :3] * 255 + 128) >> 8
    want[counts == 0] = pal.inside
    assert np.array_equal(flat, want) and (counts == 0).any() and (counts > 0).any()


def test_refusals_leave_the_output_untouched(gpu):
    import torch
    view = View(-2.0, -2.0, 4.0, 4.0, 16, 16)
    cv = gpu._cview(view, None)
    guard = 64
    dn, dd, dc = _device_buffers(torch, 256, guard)
    img = torch.full((256 + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pn, pd, pc, pi = dn[2 * guard:].data_ptr(), dd[guard:].data_ptr(), dc[guard:].data_ptr(), img[guard:].data_ptr()
    launch = gpu._lib.mbk_view_launch_normal
    assert launch(gpu._h, C.byref(cv), 100, L.MBK_KERNEL_DEFAULT, pc, None, pd, None) == L.MBK_ERR_INVALID      # NULL normals
    with pytest.raises(MbkError):
        gpu.launch_view_normals(view, 100, d_normals=0, d_counts=pc)
    for kernel in KERNELS:
        for flag in (L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, 0x1, 0x2, 0x4000, 0x80000000):
            assert launch(gpu._h, C.byref(cv), 100, L.KERNELS[kernel] | flag, pc, pn, pd, None) == L.MBK_ERR_INVALID, (kernel, flag)
    for kernel in ("simple", "refill"):
        with pytest.raises(MbkError):
            gpu.launch_view_normals(view, 100, d_normals=pn, d_counts=pc, kernel=kernel)
        with pytest.raises(MbkError):
            gpu.compute_view_normals(view, 100, kernel=kernel)
    assert launch(gpu._h, C.byref(cv), 100, 0x600, pc, pn, pd, None) == L.MBK_ERR_INVALID                         # unknown selector
    with pytest.raises(MbkError):
        gpu.launch_view_normals(view, 2 ** 31, d_normals=pn)
    with pytest.raises(MbkError):
        gpu.launch_view_normals(view, 100, d_normals=pn, window=(10, 0, 7, 16))
    with pytest.raises(MbkError):
        gpu.launch_view_normals(View(2.0 ** 500, 0.0, 2.0 ** 500, 1.0, 4, 4), 100, d_normals=pn)
    assert launch(gpu._h, None, 100, L.MBK_KERNEL_DEFAULT, None, pn, None, None) == L.MBK_ERR_INVALID
    hn, hc = np.full(512, -1.0), np.full(256, -3, np.int32)
    compute = gpu._lib.mbk_view_compute_normal
    assert compute(gpu._h, C.byref(cv), 100, 0, hc.ctypes.data, None, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, None, 100, 0, hc.ctypes.data, hn.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 100, L.MBK_PRECISION_F32, hc.ctypes.data, hn.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 2 ** 31, 0, hc.ctypes.data, hn.ctypes.data, None, None) == L.MBK_ERR_INVALID
    # the render calls: what a smooth render refuses, and the spec's own ranges
    pal = _render_palette()
    rl, rc = gpu._lib.mbk_view_relief_render_launch, gpu._lib.mbk_view_relief_render_compute
    himg = np.full((16, 16, 4), 7, np.uint8)
    ok = pal.relief_spec(1)
    bad_specs = [pal.relief_spec(5), pal.relief_spec(1, light=(1.5, 0.0)), pal.relief_spec(1, light=(0.0, math.nan)),
                 pal.relief_spec(1, light=(math.inf, 0.0)), pal.relief_spec(1, height=-0.5), pal.relief_spec(1, height=2.0 ** 10 + 1),
                 pal.relief_spec(1, height=math.nan), pal.relief_spec(1, height=math.inf),
                 Palette(pal.entries[:1]).relief_spec(1), Palette(pal.entries, scale=0.0).relief_spec(1),
                 Palette(pal.entries, scale=2.0 ** 21).relief_spec(1), Palette(pal.entries, offset=math.nan).relief_spec(1)]
    no_palette = pal.relief_spec(1)
    no_palette.palette = None
    for spec in bad_specs + [no_palette]:
        assert rl(gpu._h, C.byref(cv), 100, 0, C.byref(spec), pi, None) == L.MBK_ERR_INVALID
        assert rc(gpu._h, C.byref(cv), 100, 0, C.byref(spec), himg.ctypes.data, None) == L.MBK_ERR_INVALID
    assert rl(gpu._h, C.byref(cv), 100, 0, None, pi, None) == rc(gpu._h, C.byref(cv), 100, 0, None, himg.ctypes.data, None) == L.MBK_ERR_INVALID
    assert rl(gpu._h, C.byref(cv), 100, 0, C.byref(ok), None, None) == rc(gpu._h, C.byref(cv), 100, 0, C.byref(ok), None, None) == L.MBK_ERR_INVALID
    assert rl(gpu._h, None, 100, 0, C.byref(ok), pi, None) == L.MBK_ERR_INVALID
    for flags in (L.MBK_PRECISION_F32, L.KERNELS["simple"], L.KERNELS["refill"], 0x600, L.MBK_LAZY_UNIFORM, 0x1):
        assert rl(gpu._h, C.byref(cv), 100, flags, C.byref(ok), pi, None) == L.MBK_ERR_INVALID, flags
        assert rc(gpu._h, C.byref(cv), 100, flags, C.byref(ok), himg.ctypes.data, None) == L.MBK_ERR_INVALID, flags
    assert rl(gpu._h, C.byref(cv), 2 ** 31, 0, C.byref(ok), pi, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.render_view_relief(view, 100, palette=pal, window=(10, 0, 7, 16))
    with pytest.raises(MbkError):
        gpu.render_view_relief(view, 100, palette=pal, height=-1.0)
    torch.cuda.synchronize()
    assert (dn.cpu().numpy() == -77.0).all() and (dd.cpu().numpy() == -78.0).all() and (dc.cpu().numpy() == -5).all()
    assert (img.cpu().numpy() == 0x5A5A5A5A).all() and (himg == 7).all() and (hn == -1.0).all() and (hc == -3).all()
    # and the accepted call right after them works
    out, _ = gpu.render_view_relief(view, 100, palette=pal)
    assert out.shape == (16, 16, 4)
