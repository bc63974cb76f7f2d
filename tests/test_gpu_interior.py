"""Interior views on the GPU (include/mbk.h, "Interior views"): counts, periods and interior distance estimates held bit for bit
to the numpy model of the contract (tests/interior_model.py), through every accepted selector, windows, device pointers with
guard bands, renders and refusals."""
import ctypes as C

import numpy as np
import pytest

import interior_model as M
from distributedmandelbrot_amd import MbkError, View
from distributedmandelbrot_amd import _lib as L

pytestmark = pytest.mark.gpu

KERNELS = ["default", "scan", "group"]
FULL = ((-2.0, -1.5, 3.0, 3.0, 61, 45), 600)
# 0.02 wide around (-0.745, 0.11): boundary blocks with mixed lanes, and unknown pixels that run to the end
SEAHORSE = ((-0.755, 0.11 - 0.01 * 64 / 96, 0.02, 0.02 * 64 / 96, 96, 64), 2000)
_MODEL = {}


def _model(v, mrd):
    if (v, mrd) not in _MODEL:
        _MODEL[(v, mrd)] = M.view(v, mrd)
    return _MODEL[(v, mrd)]


def _assert_equal(period, de, counts, m, what):
    assert np.array_equal(counts, m["n"]), (what, int((counts != m["n"]).sum()))
    assert np.array_equal(period, m["period"]), (what, int((period != m["period"]).sum()))
    assert np.array_equal(de.view(np.uint64), m["de"].view(np.uint64)), (what, int((de != m["de"]).sum()))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", [FULL, SEAHORSE], ids=["full", "seahorse"])
def test_equals_the_model_with_every_selector(gpu, case, kernel):
    v, mrd = case
    m = _model(v, mrd)
    inside = m["n"] == 0
    assert inside.any() and (~inside).any() and (m["period"][inside] > 0).any()
    if case is SEAHORSE:
        assert (m["period"][inside] == 0).any() and len(np.unique(m["period"])) >= 3
    period, de, counts, st = gpu.compute_view_interior(View(*v), mrd, kernel=kernel)
    assert period.dtype == np.int32 and de.dtype == np.float64 and counts.dtype == np.int32
    _assert_equal(period, de, counts, m, kernel)
    assert not np.isnan(de).any() and (de >= 0.0).all() and (de[~inside] == 0.0).all() and (period[~inside] == 0).all()
    ref, _, st_ref = gpu.compute_view(View(*v), mrd, want_bytes=False, kernel=kernel)
    assert np.array_equal(counts, ref)
    assert (st.never_pixels, st.pixel_iterations) == (st_ref.never_pixels, st_ref.pixel_iterations)
    assert st.never_pixels == int(inside.sum())


def test_window_equals_the_same_pixels_of_the_whole_view(gpu):
    v, mrd = SEAHORSE
    m = _model(v, mrd)
    for window in ((3, 5, 50, 27), (89, 57, 7, 7), (0, 63, 96, 1), (95, 0, 1, 64)):
        c0, r0, nc, nr = window
        period, de, counts, st = gpu.compute_view_interior(View(*v), mrd, window=window)
        cut = {k: a[r0:r0 + nr, c0:c0 + nc] for k, a in m.items()}
        _assert_equal(period, de, counts, cut, window)
        assert st.never_pixels == int((cut["n"] == 0).sum())


def test_all_exterior_and_all_interior_views(gpu):
    period, de, counts, st = gpu.compute_view_interior(View(1.0, 1.0, 0.5, 0.5, 19, 11), 300)
    assert (counts > 0).all() and not period.any() and not de.any() and st.never_pixels == 0
    v, mrd = (-0.2, -0.15, 0.3, 0.3, 21, 13), 500
    period, de, counts, st = gpu.compute_view_interior(View(*v), mrd)
    _assert_equal(period, de, counts, _model(v, mrd), "interior")
    assert not counts.any() and (period == 1).all() and (de > 0.2).all() and st.never_pixels == counts.size


@pytest.mark.parametrize("mrd", [0, 1, 2, 3, 4])
def test_shallow_mrd(gpu, mrd):
    v = (-2.0, -1.5, 3.0, 3.0, 13, 13)     # holds (-0.5, 0) and (0.25, 0); a second view holds c = (-1, 0) and (0, 0)
    for v in (v, (-1.0, -1.0, 1.0, 2.0, 9, 9)):
        period, de, counts, st = gpu.compute_view_interior(View(*v), mrd)
        _assert_equal(period, de, counts, M.view(v, mrd), (v, mrd))
    if mrd < 2:
        assert not period.any() and not de.any() and not counts.any()
    else:
        assert (period[4, 8], de[4, 8]) == (1, 0.5)                       # c = (0, 0)
        assert (period[4, 0], de[4, 0]) == ((2, 0.25) if mrd >= 4 else (0, 0.0))      # c = (-1, 0)


def _buffers(torch, px, guard):
    return (torch.full((px + 2 * guard,), -5, dtype=torch.int32, device="cuda:0"),
            torch.full((px + 2 * guard,), -6, dtype=torch.int32, device="cuda:0"),
            torch.full((px + 2 * guard,), -77.0, dtype=torch.float64, device="cuda:0"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_launch_on_a_stream_with_every_pointer_combination_and_guard_bands(gpu, kernel):
    import torch
    v, mrd = FULL
    m = _model(v, mrd)
    guard = 512
    stream = torch.cuda.Stream(device="cuda:0")
    for window in (None, (5, 3, 43, 29)):
        c0, r0, nc, nr = window or (0, 0, v[4], v[5])
        cut = {k: a[r0:r0 + nr, c0:c0 + nc] for k, a in m.items()}
        px = nc * nr
        combos = [(wc, wp, wd) for wc in (True, False) for wp, wd in ((True, True), (True, False), (False, True))]
        bufs = [_buffers(torch, px, guard) for _ in combos]
        torch.cuda.synchronize()
        for (dc, dp, dd), (wc, wp, wd) in zip(bufs, combos):
            gpu.launch_view_interior(View(*v), mrd, d_counts=dc[guard:].data_ptr() if wc else 0, d_period=dp[guard:].data_ptr() if wp else 0,
                                     d_distance=dd[guard:].data_ptr() if wd else 0, stream=stream.cuda_stream, window=window, kernel=kernel)
        stream.synchronize()
        for (dc, dp, dd), wanted in zip(bufs, combos):
            for buf, want, name, sentinel in zip((dc, dp, dd), wanted, ("n", "period", "de"), (-5, -6, -77.0)):
                h = buf.cpu().numpy()
                assert (h[:guard] == sentinel).all() and (h[guard + px:] == sentinel).all(), (window, wanted, name)
                if want:
                    assert np.array_equal(h[guard:guard + px].reshape(nr, nc).view(np.uint32 if name != "de" else np.uint64),
                                          np.ascontiguousarray(cut[name]).view(np.uint32 if name != "de" else np.uint64)), (window, wanted, name)
                else:
                    assert (h == sentinel).all(), (window, wanted, name)
    # the synchronous form takes the same combinations
    for wc, wp, wd in ((False, True, True), (True, False, True), (True, True, False), (False, False, True)):
        period, de, counts, _ = gpu.compute_view_interior(View(*v), mrd, kernel=kernel, want_counts=wc, want_period=wp, want_distance=wd)
        assert (counts is None) == (not wc) and (period is None) == (not wp) and (de is None) == (not wd)
        for got, name in ((counts, "n"), (period, "period"), (de, "de")):
            assert got is None or np.array_equal(got, m[name]), (wc, wp, wd, name)


def test_refusals_write_nothing(gpu):
    import torch
    view = View(-2.0, -2.0, 4.0, 4.0, 16, 16)
    cv = gpu._cview(view, None)
    guard = 64
    dc, dp, dd = _buffers(torch, 256, guard)
    torch.cuda.synchronize()
    pc, pp, pd = dc[guard:].data_ptr(), dp[guard:].data_ptr(), dd[guard:].data_ptr()
    launch, compute = gpu._lib.mbk_view_interior_launch, gpu._lib.mbk_view_interior_compute
    hc, hp, hd = np.full(256, -5, np.int32), np.full(256, -6, np.int32), np.full(256, -77.0)
    bad_flags = [L.KERNELS["asm"], L.KERNELS["simple"], L.KERNELS["refill"], 0x600, L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_DEEP_BLA,
                 L.MBK_WANT_COUNTS, L.MBK_WANT_BYTES, L.KERNELS["group"] | L.MBK_PRECISION_F32, 0x10000]
    for flags in bad_flags:
        assert launch(gpu._h, C.byref(cv), 100, flags, pc, pp, pd, None) == L.MBK_ERR_INVALID, hex(flags)
        assert compute(gpu._h, C.byref(cv), 100, flags, hc.ctypes.data, hp.ctypes.data, hd.ctypes.data, None) == L.MBK_ERR_INVALID, hex(flags)
    assert launch(gpu._h, C.byref(cv), 100, 0, pc, None, None, None) == L.MBK_ERR_INVALID          # both value pointers NULL
    assert compute(gpu._h, C.byref(cv), 100, 0, hc.ctypes.data, None, None, None) == L.MBK_ERR_INVALID
    assert launch(gpu._h, None, 100, 0, pc, pp, pd, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, None, 100, 0, hc.ctypes.data, hp.ctypes.data, hd.ctypes.data, None) == L.MBK_ERR_INVALID
    assert launch(None, C.byref(cv), 100, 0, pc, pp, pd, None) == L.MBK_ERR_INVALID
    for kernel in ("asm", "simple", "refill"):
        with pytest.raises(MbkError):
            gpu.compute_view_interior(view, 100, kernel=kernel)
    with pytest.raises(MbkError):
        gpu.launch_view_interior(view, 2 ** 31, d_period=pp, d_distance=pd)
    with pytest.raises(MbkError):
        gpu.launch_view_interior(view, 100, d_period=pp, d_distance=pd, window=(10, 0, 7, 16))       # whatever mbk_view_launch refuses
    with pytest.raises(MbkError):
        gpu.launch_view_interior(View(2.0 ** 500, 0.0, 2.0 ** 500, 1.0, 4, 4), 100, d_period=pp, d_distance=pd)
    with pytest.raises(MbkError):
        gpu.launch_view_interior(View(-2.0, -2.0, 4.0, 4.0, 0, 16), 100, d_period=pp, d_distance=pd)
    torch.cuda.synchronize()
    assert (dc.cpu().numpy() == -5).all() and (dp.cpu().numpy() == -6).all() and (dd.cpu().numpy() == -77.0).all()
    assert (hc == -5).all() and (hp == -6).all() and (hd == -77.0).all()


def _finer(v, s):
    return v[:4] + (v[4] * s, v[5] * s)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_render_equals_the_model(gpu, s):
    import torch
    v, mrd = (-2.0, -1.25, 2.75, 2.5, 61, 45), 300
    w, h = v[4], v[5]
    view = View(*v)
    m = _model(_finer(v, s), mrd)
    pal = np.random.RandomState(11).randint(1, 256, (7, 4)).astype(np.uint8)
    unknown, outside = (1, 2, 3, 4), (250, 240, 230, 220)
    pitch = v[2] / (w - 1)
    for scale, plen in ((1.0 / (3.0 * pitch), 7), (2.0 ** 80, 7), (1.0 / (3.0 * pitch), 1)):
        want = M.render(pal[:plen], unknown, outside, scale, s, m["n"], m["period"], m["de"])
        assert len(np.unique(want.reshape(-1, 4), axis=0)) > (20 if plen > 1 and scale < 1e20 else 3)
        kw = dict(palette=pal[:plen], scale=scale, supersample=s, unknown=unknown, outside=outside)
        for rows in (0, 5):
            img, st = gpu.render_view_interior(view, mrd, max_band_rows=rows, **kw)
            assert img.shape == (h, w, 4) and np.array_equal(img, want), (s, scale, plen, rows, int((img != want).any(axis=2).sum()))
            assert st.never_pixels == int((m["n"] == 0).sum())
            assert st.pixel_iterations == int(np.where(m["n"] > 0, m["n"], mrd - 1).astype(np.int64).sum())
    window = (7, 9, 33, 21)
    img, _ = gpu.render_view_interior(view, mrd, window=window, kernel="group", **kw)
    assert np.array_equal(img, want[9:30, 7:40])
    d = torch.full((h * w + 256,), 0x01010101, dtype=torch.int32, device="cuda:0")
    gpu.launch_render_view_interior(view, mrd, d_rgba=d.data_ptr(), max_band_rows=5, **kw)
    torch.cuda.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and (hd[h * w:] == 0x01010101).all()


def test_render_refusals_write_nothing(gpu):
    import torch
    view = View(-2.0, -1.5, 3.0, 3.0, 32, 32)
    cv = gpu._cview(view, None)
    pal = np.full((3, 4), 9, np.uint8)
    out = np.full((32, 32, 4), 7, np.uint8)
    d = torch.full((32 * 32,), 0x01010101, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    compute, launch = gpu._lib.mbk_view_interior_render_compute, gpu._lib.mbk_view_interior_render_launch

    def spec(s=1, palette=pal.ctypes.data, n=3, scale=1.0):
        return L.mbk_interior_render_spec(s, palette, n, (C.c_uint8 * 4)(), (C.c_uint8 * 4)(), scale, 0)

    good = spec()
    for flags in (L.KERNELS["asm"], L.KERNELS["simple"], L.KERNELS["refill"], L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_DEEP_BLA,
                  L.MBK_WANT_BYTES):
        assert compute(gpu._h, C.byref(cv), 100, flags, C.byref(good), out.ctypes.data, None) == L.MBK_ERR_INVALID, hex(flags)
        assert launch(gpu._h, C.byref(cv), 100, flags, C.byref(good), d.data_ptr(), None) == L.MBK_ERR_INVALID, hex(flags)
    for bad in (spec(s=5), spec(s=0), spec(palette=None), spec(n=0), spec(n=65537), spec(scale=0.0), spec(scale=2.0 ** 81),
                spec(scale=float("inf")), spec(scale=float("nan"))):
        assert compute(gpu._h, C.byref(cv), 100, 0, C.byref(bad), out.ctypes.data, None) == L.MBK_ERR_INVALID
        assert launch(gpu._h, C.byref(cv), 100, 0, C.byref(bad), d.data_ptr(), None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 100, 0, None, out.ctypes.data, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 100, 0, C.byref(good), None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, None, 100, 0, C.byref(good), out.ctypes.data, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 2 ** 31, 0, C.byref(good), out.ctypes.data, None) == L.MBK_ERR_INVALID
    assert launch(gpu._h, C.byref(cv), 100, 0, C.byref(good), d.data_ptr() + 1, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.render_view_interior(view, 100, palette=pal, window=(30, 0, 3, 32))
    torch.cuda.synchronize()
    assert (out == 7).all() and (d.cpu().numpy() == 0x01010101).all()
    img, _ = gpu.render_view_interior(view, 100, palette=pal)
    assert img.shape == (32, 32, 4)
