"""Interior views on the GPU (include/mbk.h, "Interior views"): counts, periods and interior distance estimates held bit for bit
to the numpy model of the contract (tests/interior_model.py), through every accepted selector, windows, device pointers with
guard bands, renders and refusals; the literal-doubling kernel on the hazard views of tests/test_interior.py (rows with a
subnormal c_i, where the fused kernel would give other periods); mrd at the edges of the Brent windows; degenerate and backwards
axes; and the device's periods and de held to the mpmath truth (tests/interior_truth.py) with no model in between."""
import ctypes as C

import numpy as np
import pytest

import interior_model as M
import interior_truth as T
from test_interior import HAZARD, HAZARD_CASES, HAZARD_MIXED, differing_pixels
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


@pytest.mark.parametrize("case", HAZARD_CASES, ids=[f"{i}-{mrd}" for i, (_, t) in enumerate(HAZARD) for mrd in t])
def test_hazard_views_equal_the_literal_model(gpu, case):
    """Views with rows 0 < |c_i| < 2^-900 run interior_kernel<false>.  The fused kernel would differ from the model on as many
    pixels as the table says (tests/test_interior.py::test_hazard_claims); the message carries the count per selector."""
    v, mrd = case
    m = _model(v, mrd)
    inside = m["n"] == 0
    assert (m["period"] > 0).any() and (~inside).any()
    ref, _, st_ref = gpu.compute_view(View(*v), mrd, want_bytes=False)
    assert np.array_equal(ref, m["n"])
    wrong = {}
    for kernel in KERNELS:
        period, de, counts, st = gpu.compute_view_interior(View(*v), mrd, kernel=kernel)
        assert np.array_equal(counts, m["n"]), kernel
        assert (st.never_pixels, st.pixel_iterations) == (st_ref.never_pixels, st_ref.pixel_iterations)
        assert st.never_pixels == int(inside.sum())
        assert not np.isnan(de).any() and (de >= 0.0).all()
        wrong[kernel] = differing_pixels((period, de), m)
    assert wrong == dict.fromkeys(KERNELS, 0), (v, mrd, "pixels that differ from the literal model", wrong)


def test_windows_of_a_view_with_one_tiny_row_keep_their_bits(gpu):
    """HAZARD_MIXED: row 0 alone needs the literal kernel, so the whole view and the windows that hold row 0 take it and the
    window of rows 1..7 takes the fused one.  The kernel changes between them and the bits must not."""
    v = HAZARD_MIXED
    for mrd in (65, 257):
        m = _model(v, mrd)
        fused_row0 = M.view(v, mrd, window=(0, 0, 96, 1), fma=True)
        assert differing_pixels(fused_row0, {k: a[0:1] for k, a in m.items()}) == dict(HAZARD)[v][mrd]      # the test has power
        wrong = {}
        for window in ((0, 0, 96, 1), (0, 1, 96, 7), (0, 0, 96, 3), (37, 0, 30, 5), (90, 1, 6, 2)):
            c0, r0, nc, nr = window
            cut = {k: a[r0:r0 + nr, c0:c0 + nc] for k, a in m.items()}
            for kernel in ("default", "group"):
                period, de, counts, st = gpu.compute_view_interior(View(*v), mrd, window=window, kernel=kernel)
                assert np.array_equal(counts, cut["n"]) and st.never_pixels == int((cut["n"] == 0).sum()), (mrd, window, kernel)
                wrong[window + (kernel,)] = differing_pixels((period, de), cut)
        assert not any(wrong.values()), (mrd, wrong)


BRENT_EDGES = [32, 33, 34, 64, 65, 66, 128, 129, 130, 1024, 1025, 1026]


@pytest.mark.parametrize("mrd", BRENT_EDGES)
def test_mrd_at_the_brent_window_edges(gpu, mrd):
    """The reference moves at steps 1, 3, 7, ... 2^j - 1: mrd - 1 = the last step run lies just before, on and just after one.
    On the boundary waves of these views some lanes hit on that step and others run out."""
    settled = {}
    for name, v in (("full", FULL[0]), ("seahorse", SEAHORSE[0])):
        m = _model(v, mrd)
        period, de, counts, st = gpu.compute_view_interior(View(*v), mrd)
        _assert_equal(period, de, counts, m, (name, mrd))
        assert st.never_pixels == int((m["n"] == 0).sum())
        settled[name] = int((m["period"] > 0).sum())
        if mrd > 32:      # a longer search keeps every hit of a shorter one
            before = _model(v, BRENT_EDGES[BRENT_EDGES.index(mrd) - 1])
            assert (m["period"][before["period"] > 0] == before["period"][before["period"] > 0]).all()
    full = _model(FULL[0], mrd)
    assert settled["full"] >= 3 and ((full["n"] == 0) & (full["period"] == 0)).any() and full["at_window"].any()
    if mrd in (33, 65, 129):      # the first step of a new window finds hits of its own (24 / 62 / 132 settled against 3 / 26 / 93)
        assert settled["full"] > int((_model(FULL[0], mrd - 1)["period"] > 0).sum())
    if mrd >= 1024:
        assert settled["seahorse"] == 10


DEGENERATE = [((-2.0, 0.0, 2.5, 0.0, 101, 1), 56), ((-0.1, -1.2, 0.0, 2.4, 1, 77), 43), ((0.5, 1.2, -2.5, -2.4, 31, 21), 98),
              ((-1.0, 0.0, 0.0, 0.0, 1, 1), 1), ((-0.75, 0.1, 0.0, 0.0, 5, 4), 0)]


@pytest.mark.parametrize("v,settled", DEGENERATE, ids=["1-high", "1-wide", "backwards", "1x1", "zero-ranges"])
def test_degenerate_and_backwards_axes(gpu, v, settled):
    """np.linspace is the library's axis on these too (a zero range repeats the start, a negative one runs backwards, one sample
    is the start), so the model takes its coordinates as for every other view."""
    mrd = 300
    m = _model(v, mrd)
    assert int((m["period"] > 0).sum()) == settled
    for kernel in ("default", "group"):
        period, de, counts, st = gpu.compute_view_interior(View(*v), mrd, kernel=kernel)
        assert period.shape == (v[5], v[4])
        _assert_equal(period, de, counts, m, (v, kernel))
        assert st.never_pixels == int((m["n"] == 0).sum())
    if v[4] * v[5] > 1:
        window = (v[4] // 2, v[5] // 2, 1, 1)
        period, de, counts, _ = gpu.compute_view_interior(View(*v), mrd, window=window)
        _assert_equal(period, de, counts, {k: a[window[1]:window[1] + 1, window[0]:window[0] + 1] for k, a in m.items()}, (v, window))


@pytest.mark.parametrize("case", [T.SEAHORSE, T.FULL64], ids=["seahorse", "full64"])
def test_device_equals_the_truth(gpu, case):
    """The device's periods and de against the mpmath truth of the multiplier, with no model in between: every settled pixel
    converges, has the exact minimal period the device says, is attracting and lies within K0."""
    v, mrd = case
    period, de, counts, _ = gpu.compute_view_interior(View(*v), mrd)
    xr, xi = M.axes(v)
    cr, ci = np.meshgrid(xr, xi)
    w = T.assert_truth(cr, ci, period, de, mrd, f"device {v[4]} x {v[5]} at mrd {mrd}")
    assert w["settled"] == int((period > 0).sum()) == (50 if case is T.SEAHORSE else 586)
    assert (period[counts > 0] == 0).all() and (de[period == 0] == 0.0).all()


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


def test_launch_on_a_stream_on_a_hazard_view(gpu):
    import torch
    v, mrd = HAZARD[0][0], 65
    m = _model(v, mrd)
    guard = 512
    stream = torch.cuda.Stream(device="cuda:0")
    windows = (None, (3, 1, 50, 5))
    bufs = []
    for window in windows:
        c0, r0, nc, nr = window or (0, 0, v[4], v[5])
        bufs.append(_buffers(torch, nc * nr, guard))
    torch.cuda.synchronize()
    for window, (dc, dp, dd) in zip(windows, bufs):
        gpu.launch_view_interior(View(*v), mrd, d_counts=dc[guard:].data_ptr(), d_period=dp[guard:].data_ptr(),
                                 d_distance=dd[guard:].data_ptr(), stream=stream.cuda_stream, window=window)
    stream.synchronize()
    for window, triple in zip(windows, bufs):
        c0, r0, nc, nr = window or (0, 0, v[4], v[5])
        px = nc * nr
        cut = {k: a[r0:r0 + nr, c0:c0 + nc] for k, a in m.items()}
        host = [b.cpu().numpy() for b in triple]
        for h, sentinel in zip(host, (-5, -6, -77.0)):
            assert (h[:guard] == sentinel).all() and (h[guard + px:] == sentinel).all(), window
        counts, period, de = (h[guard:guard + px].reshape(nr, nc) for h in host)
        assert np.array_equal(counts, cut["n"]), window
        assert differing_pixels((period, de), cut) == 0, (window, differing_pixels((period, de), cut))


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


@pytest.mark.parametrize("s", [1, 2, 3, 4, 8])
def test_render_equals_the_model(gpu, s):
    import torch
    v, mrd = (-2.0, -1.25, 2.75, 2.5) + ((61, 45) if s <= 3 else (21, 15)), 300      # (s = 4 and 8: 64 samples per pixel at the most)
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
    window = (7, 9, 33, 21) if s <= 3 else (3, 2, 11, 9)
    img, _ = gpu.render_view_interior(view, mrd, window=window, kernel="group", **kw)
    assert np.array_equal(img, want[window[1]:window[1] + window[3], window[0]:window[0] + window[2]])
    d = torch.full((h * w + 256,), 0x01010101, dtype=torch.int32, device="cuda:0")
    gpu.launch_render_view_interior(view, mrd, d_rgba=d.data_ptr(), max_band_rows=5, **kw)
    torch.cuda.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and (hd[h * w:] == 0x01010101).all()


@pytest.mark.parametrize("s", [1, 2])
def test_render_with_a_palette_too_large_for_lds(gpu, s):
    """16385 entries: one more than the resolve kernel keeps in LDS, so the interior rule reads the palette from global memory."""
    v, mrd = (-2.0, -1.25, 2.75, 2.5, 61, 45), 300
    m = _model(_finer(v, s), mrd)
    pal = np.random.RandomState(12).randint(1, 256, (16385, 4)).astype(np.uint8)
    used = np.unique(m["period"][m["period"] > 0]) - 1
    assert len(used) >= 3 and len(np.unique(pal[used], axis=0)) >= 3      # at least three distinct entries are looked up
    unknown, outside = (1, 2, 3, 4), (250, 240, 230, 220)
    for scale in (1.0 / (3.0 * v[2] / (v[4] - 1)), 2.0 ** 80):
        want = M.render(pal, unknown, outside, scale, s, m["n"], m["period"], m["de"])
        small = M.render(pal[:7], unknown, outside, scale, s, m["n"], m["period"], m["de"])
        assert (want != small).any()                                          # entries past the seventh show in the image
        for rows in (0, 5):
            img, st = gpu.render_view_interior(View(*v), mrd, palette=pal, scale=scale, supersample=s, unknown=unknown, outside=outside,
                                               max_band_rows=rows)
            assert np.array_equal(img, want), (s, scale, rows, int((img != want).any(axis=2).sum()))
            assert st.never_pixels == int((m["n"] == 0).sum())


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_render_of_a_hazard_view_equals_the_literal_model(gpu, s):
    """One tiny row among the samples: the whole render and the band that holds row 0 take the literal kernel, the other bands
    of max_band_rows = 3 the fused one."""
    v, mrd = (-2.0, 1e-310, 2.5, 0.7, 48, 8), 65
    pal = np.random.RandomState(11).randint(1, 256, (7, 4)).astype(np.uint8)
    unknown, outside = (1, 2, 3, 4), (250, 240, 230, 220)
    m, fused = _model(_finer(v, s), mrd), M.view(_finer(v, s), mrd, fma=True)
    want = M.render(pal, unknown, outside, 2.0 ** 80, s, m["n"], m["period"], m["de"])
    other = M.render(pal, unknown, outside, 2.0 ** 80, s, fused["n"], fused["period"], fused["de"])
    differ = int((want != other).any(axis=2).sum())
    assert differ >= 1 and differ == {1: 3, 2: 3, 4: 3, 8: 4}[s]             # what the fused kernel would get wrong
    for rows in (0, 3):
        for kernel in ("default", "group"):
            img, st = gpu.render_view_interior(View(*v), mrd, palette=pal, scale=2.0 ** 80, supersample=s, unknown=unknown, outside=outside,
                                               max_band_rows=rows, kernel=kernel)
            assert np.array_equal(img, want), (s, rows, kernel, "output pixels that differ", int((img != want).any(axis=2).sum()))
            assert st.never_pixels == int((m["n"] == 0).sum())


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
