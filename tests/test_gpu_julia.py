"""GPU tests of Julia views (include/mbk.h, "Julia views"): counts and bytes bit for bit against the numpy model of
tests/julia_model.py, nu within the smooth allowance of the correctly rounded value at the model's mag; every kernel and
option agrees; windows, bands and the three call forms agree; renders and histograms equal their host twins; refusals write
nothing."""
import ctypes as C

import numpy as np
import pytest

import julia_model as J
import smooth_truth as T
from distributedmandelbrot_amd import View, sharding
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import Palette, equalize_lut, resolve_host

pytestmark = pytest.mark.gpu

NAMED = [(-1.0, 0.0), (-0.75, 0.0), (0.25, 0.0), (0.0, 1.0), (-0.8, 0.156), (0.0, 0.0)]
OUTSIDE = [(1.5, 1.5)]
RING = [(-2.0, 0.0), (-2.0 + 1e-10, 0.0), (-2.0 - 1e-10, 0.0)]
# Douady's rabbit (period-3 bulb) and a point of the main cardioid: connected sets with an interior and c_i != 0, the only class
# whose interior runs through the grouped loop and is retired by the cycle test (c_i = 0 takes the literal per-step loop,
# -0.8+0.156i lies outside the Mandelbrot set, i is a dendrite)
INTERIOR = [(-0.123, 0.745), (-0.5, 0.5)]
PARAMS = NAMED + OUTSIDE + RING + INTERIOR

# (start_r, start_i, range_r, range_i, width, height): 64 .. 1024 pixels, sizes that are no multiples of 8
VIEWS = [
    (-1.7, -1.3, 3.4, 2.6, 37, 27),       # 999 pixels
    (-1.6, -1.2, 3.2, 2.4, 9, 11),        # 99
    (-2.0, 0.3, 4.0, 0.0, 101, 1),        # 1 high
    (0.1, -1.9, 0.0, 3.8, 1, 77),         # 1 wide
    (1.6, 1.2, -3.2, -2.4, 31, 21),       # both axes backwards
]
# hazard views: every row subnormal (c_i = 0 keeps zi tiny; on the real axis of a chaotic parameter it grows until the orbit
# escapes, at a step the first subnormal products decide -- tests/test_julia.py shows the fused doubling would differ)
HAZARD_VIEWS = [
    (-1.5, -3e-323, 3.0, 6e-323, 29, 13),
    (0.3, 5e-324, 1.2, 1e-321, 23, 9),
]
HAZARD_PARAMS = [(-1.8, 0.0), (-1.9, 0.0), (-0.75, 0.0), (-1.0, 0.0)]
MRD = 3000

BYTES_PAL = Palette.viewer()
SMOOTH_PAL = Palette.cosine(777, period=5.5, inside=(9, 8, 7, 255))
EQ_PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255)).for_equalized()
OPTIONS = ("group_steps", "exact_steps", "cycle_detect", "cycle_window", "wave_limit")


def _torch():
    import torch
    return torch


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


@pytest.fixture()
def options(gpu):
    """The options a test changes are put back afterwards."""
    saved = {k: gpu.get_option(k) for k in OPTIONS}
    yield gpu
    for k, v in saved.items():
        gpu.set_option(k, v)


def check_against_model(gpu, v, c, mrd, what, kernel="default"):
    view = View(*v)
    counts, byts, nu, st = gpu.compute_julia_view(view, c, mrd, want_smooth=True, kernel=kernel)
    wn, wmag = J.julia_view(v, c, mrd)
    assert np.array_equal(counts, wn), (what, int((counts != wn).sum()))
    assert np.array_equal(byts, J.quantise(wn, mrd)), what
    T.assert_within(nu, wn, wmag, what)
    assert st.pixel_iterations == int(np.where(wn > 0, wn, mrd - 1).sum()) and st.never_pixels == int((wn == 0).sum()), what
    return counts, byts, nu


@pytest.mark.parametrize("c", PARAMS)
def test_counts_bytes_and_smooth_equal_the_model(gpu, c):
    seen = set()
    for v in VIEWS:
        for kernel in ("default", "asm", "group"):
            counts, _, _ = check_against_model(gpu, v, c, MRD, f"c={c} view={v} {kernel}", kernel)
        seen.update(np.unique(counts).tolist())
    assert len(seen) > 2, seen
    check_against_model(gpu, VIEWS[0], c, 2, f"c={c} mrd 2")
    check_against_model(gpu, VIEWS[0], c, 257, f"c={c} mrd 257")


def test_mrd_0_and_1_run_no_step(gpu):
    view = View(*VIEWS[0])
    for mrd in (0, 1):
        counts, _, nu, st = gpu.compute_julia_view(view, (-0.8, 0.156), mrd, want_bytes=False, want_smooth=True)
        assert not counts.any() and not nu.any() and st.never_pixels == counts.size
    _, byts, _, _ = gpu.compute_julia_view(view, (-0.8, 0.156), 1, want_counts=False)
    assert not byts.any()


@pytest.mark.parametrize("c", HAZARD_PARAMS)
def test_hazard_views_equal_the_literal_model(gpu, c):
    differs = 0
    for v in HAZARD_VIEWS:
        for kernel in ("default", "asm", "group"):
            check_against_model(gpu, v, c, MRD, f"hazard c={c} view={v} {kernel}", kernel)
        differs += int((J.julia_view(v, c, MRD, fma=True)[0] != J.julia_view(v, c, MRD)[0]).sum())
    if c[0] in (-1.8, -1.9):
        assert differs > 0   # the fused doubling would have stored other counts on these very views


def test_the_identity_with_the_mandelbrot_view(gpu, oracle):
    # a view whose samples hit c bit for bit (c is a sample of both axes): the pixel at c holds the Mandelbrot count of c
    for c, mrd in [((-0.75, 0.125), 500), ((0.25, 0.5), 500), ((-1.75, 0.0), 300), ((0.375, -0.25), 2000)]:
        v = (-2.0, -2.0, 4.0, 4.0, 33, 33)
        re, im = J.axes(v)
        col, row = int(np.flatnonzero(re == c[0])[0]), int(np.flatnonzero(im == c[1])[0])
        counts, _, _, _ = gpu.compute_julia_view(View(*v), c, mrd, want_bytes=False)
        assert counts[row, col] == oracle.escape(c[0], c[1], mrd), c


SWEEP_CASES = [(v, c) for v in VIEWS for c in PARAMS] + [(v, c) for v in HAZARD_VIEWS for c in HAZARD_PARAMS]


def test_kernels_and_options_agree(options):
    """Every view / parameter case of this file: asm (checked against the model), group and default store the same bits under
    every value of the options the loops read."""
    gpu = options
    retired = 0
    for v, c in SWEEP_CASES:
        view = View(*v)
        *want, st = gpu.compute_julia_view(view, c, MRD, want_smooth=True, kernel="asm")
        wn, _ = J.julia_view(v, c, MRD)
        assert np.array_equal(want[0], wn), (v, c)
        if c in INTERIOR and v == VIEWS[0]:
            assert st.never_pixels > 0, (v, c)      # lanes the cycle test can retire, under every option below
            retired += st.never_pixels

        def same(what):
            for kernel in ("default", "group"):
                *got, gst = gpu.compute_julia_view(view, c, MRD, want_smooth=True, kernel=kernel)
                for a, b in zip(got, want):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (v, c, kernel, what)
                assert (gst.pixel_iterations, gst.never_pixels) == (st.pixel_iterations, st.never_pixels), (v, c, kernel, what)

        for cyc in (0, 1):
            gpu.set_option("cycle_detect", cyc)
            for gs in (4, 8, 16, 32):
                gpu.set_option("group_steps", gs)
                for ex in (0, 8, 100):
                    gpu.set_option("exact_steps", ex)
                    same((cyc, gs, ex))
        gpu.set_option("cycle_detect", 1)
        for gs in (8, 16):
            gpu.set_option("group_steps", gs)
            for ex in (0, 8):
                gpu.set_option("exact_steps", ex)
                for win in (0, 4, 65536):
                    gpu.set_option("cycle_window", win)
                    same(("window", gs, ex, win))
        gpu.set_option("cycle_window", 32)
        gpu.set_option("group_steps", 16)
        gpu.set_option("exact_steps", 8)
        for wl in (0, 2, 5):
            gpu.set_option("wave_limit", wl)
            same(("wave_limit", wl))
        gpu.set_option("wave_limit", 0)
    assert retired > 100


def test_a_large_connected_view_asm_against_default(gpu):
    # Douady's rabbit: c in the period-3 bulb, a connected set with an interior (-0.8+0.156i lies outside the Mandelbrot set)
    view, c, mrd = View(-1.6, -1.2, 3.2, 2.4, 2048, 2048), (-0.123, 0.745), 4000
    a = gpu.compute_julia_view(view, c, mrd, want_smooth=True, kernel="asm")
    d = gpu.compute_julia_view(view, c, mrd, want_smooth=True, kernel="default")
    for x, y in zip(a[:3], d[:3]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert (a[3].pixel_iterations, a[3].never_pixels) == (d[3].pixel_iterations, d[3].never_pixels)
    # not a degenerate image: an interior, an exterior and more than a handful of escape steps (the rabbit is hyperbolic:
    # its exterior leaves within some 90 steps, so there are tens of distinct counts, not hundreds)
    assert 0 < d[3].never_pixels < view.width * view.height and len(np.unique(d[0])) > 10
    # the model on a sample of rows
    for row in (0, 700, 1024, 2047):
        wn, _ = J.julia_view((-1.6, -1.2, 3.2, 2.4, 2048, 2048), c, mrd, window=(0, row, 2048, 1))
        assert np.array_equal(d[0][row], wn[0]), row


def test_windows_bands_and_forms(gpu):
    torch = _torch()
    v, c, mrd = (-1.7, -1.3, 3.4, 2.6, 77, 53), (-0.8, 0.156), 1200
    view = View(*v)
    counts, byts, nu, st = gpu.compute_julia_view(view, c, mrd, want_smooth=True)
    wn, _ = J.julia_view(v, c, mrd)
    assert np.array_equal(counts, wn)
    assert st.pixel_iterations == int(np.where(counts > 0, counts, mrd - 1).sum()) and st.never_pixels == int((counts == 0).sum())
    assert st.rle_runs == 1 + int((byts.ravel()[1:] != byts.ravel()[:-1]).sum())
    for window in T.WINDOWS:
        c0, r0, nc, nr = window
        wc, wb, wnu, wst = gpu.compute_julia_view(view, c, mrd, window=window, want_smooth=True)
        assert np.array_equal(wc, counts[r0:r0 + nr, c0:c0 + nc]) and np.array_equal(wb, byts[r0:r0 + nr, c0:c0 + nc]), window
        assert np.array_equal(wnu.view(np.uint64), nu[r0:r0 + nr, c0:c0 + nc].view(np.uint64)), window
        assert wst.never_pixels == int((wc == 0).sum())
        # submit / wait on a slot
        sc, sb = np.full((nr, nc), -7, np.int32), np.full((nr, nc), 0xA5, np.uint8)
        gpu.submit_julia_view(2, view, c, mrd, window=window, out_counts=sc, out_bytes=sb)
        sst = gpu.wait(2)
        assert np.array_equal(sc, wc) and np.array_equal(sb, wb)
        assert (sst.pixel_iterations, sst.never_pixels, sst.rle_runs) == (wst.pixel_iterations, wst.never_pixels, wst.rle_runs)
        # launch on device buffers, guarded on both sides
        px = nr * nc
        d_c = torch.full((px + 32,), -7, dtype=torch.int32, device="cuda:0")
        d_b = torch.full((px + 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_s = torch.full((px + 32,), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        gpu.launch_julia_view(view, c, mrd, window=window, d_counts=d_c.data_ptr() + 64, d_bytes=d_b.data_ptr() + 16,
                              d_smooth=d_s.data_ptr() + 128)
        torch.cuda.synchronize()
        gc, gb, gs = d_c.cpu().numpy(), d_b.cpu().numpy(), d_s.cpu().numpy()
        assert np.array_equal(gc[16:16 + px].reshape(nr, nc), wc) and (gc[:16] == -7).all() and (gc[16 + px:] == -7).all()
        assert np.array_equal(gb[16:16 + px].reshape(nr, nc), wb) and (gb[:16] == 0xA5).all() and (gb[16 + px:] == 0xA5).all()
        assert np.array_equal(gs[16:16 + px].reshape(nr, nc).view(np.uint64), wnu.view(np.uint64))
        assert (gs[:16] == -7.0).all() and (gs[16 + px:] == -7.0).all()
    # row bands from a shared queue on one device
    for band_rows in (8, 13, 53):
        bc, bb, per_dev = sharding.render_julia_view([gpu], view, c, mrd, band_rows=band_rows)
        assert np.array_equal(bc, counts) and np.array_equal(bb, byts)
        assert per_dev[0]["pixel_iterations"] == st.pixel_iterations


@pytest.mark.parametrize("s", [1, 2, 3])
def test_renders_equal_the_host_resolve_of_the_samples(gpu, s):
    torch = _torch()
    w, h, c, mrd = 61, 45, (-0.8, 0.156), 900
    view = View(-1.7, -1.3, 3.4, 2.6, w, h)
    counts, byts, nu, st_s = gpu.compute_julia_view(_finer(view, s), c, mrd, want_smooth=True)
    for source, pal, kw in (("bytes", BYTES_PAL, {"bytes_": byts}), ("smooth", SMOOTH_PAL, {"counts": counts, "smooth": nu})):
        want = resolve_host(pal, source, s, w, h, **kw)
        img, st = gpu.render_julia_view(view, c, mrd, palette=pal, source=source, supersample=s)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (source, int((img != want).any(axis=2).sum()))
        assert len(np.unique(img.reshape(-1, 4), axis=0)) > 8
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
        banded, _ = gpu.render_julia_view(view, c, mrd, palette=pal, source=source, supersample=s, max_band_rows=7)
        assert np.array_equal(banded, img), source
        for kernel in ("asm", "group"):
            again, _ = gpu.render_julia_view(view, c, mrd, palette=pal, source=source, supersample=s, kernel=kernel, max_band_rows=16)
            assert np.array_equal(again, img), (source, kernel)
        c0, r0, nc, nr = 5, 7, 40, 30
        part, _ = gpu.render_julia_view(view, c, mrd, palette=pal, source=source, supersample=s, window=(c0, r0, nc, nr), max_band_rows=4)
        assert np.array_equal(part, img[r0:r0 + nr, c0:c0 + nc]), source
        buf = torch.full((64 + img.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gpu.launch_render_julia_view(view, c, mrd, palette=pal, d_rgba=buf.data_ptr() + 64, source=source, supersample=s, max_band_rows=9)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[64:64 + img.size].reshape(img.shape), img), source
        assert (got[:64] == 0xA5).all() and (got[64 + img.size:] == 0xA5).all()
    # equalised: the table is that of the whole view at output resolution
    hist = gpu.julia_view_histogram(view, c, mrd)
    c1 = gpu.compute_julia_view(view, c, mrd, want_bytes=False)[0]
    assert np.array_equal(hist, np.bincount(c1.ravel(), minlength=mrd).astype(np.uint64))
    table = equalize_lut(hist)
    want = resolve_host(EQ_PAL, "equalized", s, w, h, counts=counts, smooth=nu, lut=table)
    img, st = gpu.render_julia_view(view, c, mrd, palette=EQ_PAL, source="equalized", supersample=s)
    assert np.array_equal(img, want), int((img != want).any(axis=2).sum())
    assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    banded, _ = gpu.render_julia_view(view, c, mrd, palette=EQ_PAL, source="equalized", supersample=s, max_band_rows=5, window=(3, 2, 50, 41))
    assert np.array_equal(banded, img[2:43, 3:53])
    other = np.sqrt(table)
    img2, _ = gpu.render_julia_view(view, c, mrd, palette=EQ_PAL, source="equalized", supersample=s, lut=other)
    assert np.array_equal(img2, resolve_host(EQ_PAL, "equalized", s, w, h, counts=counts, smooth=nu, lut=other)) and not np.array_equal(img2, img)
    buf = torch.full((img.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_julia_view(view, c, mrd, palette=EQ_PAL, d_rgba=buf.data_ptr(), source="equalized", supersample=s, lut=table)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:img.size].reshape(img.shape), img) and (got[img.size:] == 0xA5).all()


@pytest.mark.parametrize("c", [(-0.8, 0.156), (-1.0, 0.0), (1.5, 1.5), (-2.0, 0.0)])
def test_histograms_equal_bincount(gpu, c):
    torch = _torch()
    mrd = 700
    view = View(-1.7, -1.3, 3.4, 2.6, 203, 131)
    counts = gpu.compute_julia_view(view, c, mrd, want_bytes=False)[0]
    want = np.bincount(counts.ravel(), minlength=mrd).astype(np.uint64)
    for kernel in ("default", "asm", "group"):
        hist, st = gpu.julia_view_histogram(view, c, mrd, kernel=kernel, want_stats=True)
        assert np.array_equal(hist, want), kernel
        assert st.never_pixels == int(want[0]) and st.pixel_iterations == int((np.arange(mrd) * want).sum() + (mrd - 1) * want[0])
    window = (11, 3, 150, 99)
    part = gpu.julia_view_histogram(view, c, mrd, window=window)
    assert np.array_equal(part, np.bincount(counts[3:102, 11:161].ravel(), minlength=mrd).astype(np.uint64))
    # the launch form ADDS into a device table
    d_hist = torch.from_numpy(np.full(mrd + 2, 5, np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    gpu.launch_julia_view_histogram(view, c, mrd, d_hist=d_hist.data_ptr() + 8)
    gpu.launch_julia_view_histogram(view, c, mrd, d_hist=d_hist.data_ptr() + 8, window=window)
    torch.cuda.synchronize()
    got = d_hist.cpu().numpy().view(np.uint64)
    assert got[0] == 5 and got[-1] == 5 and np.array_equal(got[1:-1], 5 + want + part)


def test_refusals_leave_the_outputs_untouched(gpu):
    torch = _torch()
    lib = L.load()
    bad = L.MBK_ERR_INVALID
    view = View(-1.7, -1.3, 3.4, 2.6, 64, 48)
    cv = gpu._cview(view, None)
    px, mrd = 64 * 48, 256
    both = L.MBK_WANT_COUNTS | L.MBK_WANT_BYTES
    counts, byts = np.full(px, -7, np.int32), np.full(px, 0xA5, np.uint8)
    nu, hist, rgba = np.full(px, -7.0), np.full(mrd, 12345, np.uint64), np.full(px * 4, 0xA5, np.uint8)

    def untouched():
        return (counts == -7).all() and (byts == 0xA5).all() and (nu == -7.0).all() and (hist == 12345).all() and (rgba == 0xA5).all()

    def compute(v=cv, c=(-0.8, 0.156), m=mrd, flags=both, pc=counts, pb=byts, ps=nu):
        ptr = [a.ctypes.data if a is not None else None for a in (pc, pb, ps)]
        return lib.mbk_julia_view_compute(gpu._h, C.byref(v) if v is not None else None, c[0], c[1], m, flags, *ptr, None)

    def submit(v=cv, c=(-0.8, 0.156), m=mrd, flags=both, slot=1):
        return lib.mbk_julia_view_submit(gpu._h, slot, C.byref(v), c[0], c[1], m, flags, counts.ctypes.data, byts.ctypes.data)

    view_cases = {
        "simple": dict(flags=both | L.MBK_KERNEL_SIMPLE), "refill": dict(flags=both | L.MBK_KERNEL_REFILL),
        "scan": dict(flags=both | L.MBK_KERNEL_SCAN), "unknown kernel": dict(flags=both | 0x700),
        "fp32": dict(flags=both | L.MBK_PRECISION_F32), "lazy uniform": dict(flags=both | L.MBK_LAZY_UNIFORM),
        "an unknown bit": dict(flags=both | 0x4000), "c NaN": dict(c=(np.nan, 0.0)), "c inf": dict(c=(0.0, -np.inf)),
        "mrd 2^31": dict(m=1 << 31), "mrd 0 with bytes": dict(m=0),
        "window exceeds the view": dict(v=gpu._cview(view, (1, 0, 64, 48))), "empty window": dict(v=gpu._cview(view, (0, 0, 0, 48))),
        "view not finite": dict(v=gpu._cview(View(np.nan, -1.3, 3.4, 2.6, 64, 48), None)),
        "view beyond 2^500": dict(v=gpu._cview(View(-1e200, -1.3, 2e200, 2.6, 64, 48), None)),
    }
    for name, kw in view_cases.items():
        assert compute(**kw) == bad and untouched(), name
        assert submit(**kw) == bad and untouched(), name
    assert compute(v=None) == bad and compute(flags=0, ps=None) == bad and compute(pc=None) == bad and compute(pb=None) == bad and untouched()
    assert submit(flags=0) == bad and submit(slot=L.MBK_SLOTS) == bad and submit(slot=-1) == bad and untouched()
    assert lib.mbk_julia_view_compute(None, C.byref(cv), -0.8, 0.156, mrd, both, counts.ctypes.data, byts.ctypes.data, None, None) == bad
    assert lib.mbk_wait(gpu._h, 1, None) == bad       # nothing was submitted

    # the launch form, on guarded device buffers
    d_c = torch.full((px,), -7, dtype=torch.int32, device="cuda:0")
    d_b = torch.full((px,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_s = torch.full((px,), -7.0, dtype=torch.float64, device="cuda:0")
    d_h = torch.full((mrd,), 12345, dtype=torch.int64, device="cuda:0")
    d_i = torch.full((px * 4,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def launch(v=cv, c=(-0.8, 0.156), m=mrd, flags=both):
        return lib.mbk_julia_view_launch(gpu._h, C.byref(v), c[0], c[1], m, flags, d_c.data_ptr(), d_b.data_ptr(), d_s.data_ptr(), None)

    for name, kw in view_cases.items():
        assert launch(**kw) == bad, name
    assert lib.mbk_julia_view_launch(gpu._h, C.byref(cv), -0.8, 0.156, mrd, both, None, d_b.data_ptr(), None, None) == bad
    assert lib.mbk_julia_view_launch(gpu._h, C.byref(cv), -0.8, 0.156, mrd, 0, None, None, None, None) == bad

    # renders: render_check's refusals, the distance sources, flags other than kernel selection
    def render(pal=SMOOTH_PAL, source="smooth", s=1, flags=0, c=(-0.8, 0.156), m=mrd, v=cv, dst=rgba, launch_form=False):
        spec = pal.spec(source, s)
        if launch_form:
            return lib.mbk_julia_view_render_launch(gpu._h, C.byref(v), c[0], c[1], m, flags, C.byref(spec), d_i.data_ptr(), None)
        return lib.mbk_julia_view_render_compute(gpu._h, C.byref(v) if v is not None else None, c[0], c[1], m, flags, C.byref(spec),
                                                 dst.ctypes.data if dst is not None else None, None)

    dist_pal = Palette.distance(view)
    render_cases = {
        "distance": dict(pal=dist_pal, source="distance"), "distance_rel": dict(pal=dist_pal, source="distance_rel"),
        "equalized without a table": dict(pal=EQ_PAL, source="equalized"), "supersample 5": dict(s=5),
        "bytes with a long palette": dict(source="bytes"), "bytes with mrd 0": dict(pal=BYTES_PAL, source="bytes", m=0),
        "fp32": dict(flags=L.MBK_PRECISION_F32), "scan": dict(flags=L.MBK_KERNEL_SCAN), "simple": dict(flags=L.MBK_KERNEL_SIMPLE),
        "an output flag": dict(flags=L.MBK_WANT_COUNTS), "c NaN": dict(c=(0.0, np.nan)), "mrd 2^31": dict(m=1 << 31),
        "window exceeds the view": dict(v=gpu._cview(view, (0, 1, 64, 48))),
    }
    for name, kw in render_cases.items():
        assert render(**kw) == bad and untouched(), name
        assert render(launch_form=True, **kw) == bad, name
    assert render(v=None) == bad and render(dst=None) == bad and untouched()
    table = np.linspace(0.0, 1.0, mrd + 2)
    spec = EQ_PAL.spec("equalized", 1)

    def eq(lut=table, n=mrd + 2, sp=spec, c=(-0.8, 0.156), flags=0):
        return lib.mbk_julia_view_render_equalized_compute(gpu._h, C.byref(cv), c[0], c[1], mrd, flags, C.byref(sp),
                                                           lut.ctypes.data if lut is not None else None, n, rgba.ctypes.data, None)

    assert eq(lut=None) == bad and eq(n=mrd + 1) == bad and eq(sp=SMOOTH_PAL.spec("smooth", 1)) == bad and untouched()
    assert eq(lut=table * 2.0) == bad and eq(c=(np.inf, 0.0)) == bad and eq(flags=L.MBK_KERNEL_REFILL) == bad and untouched()
    assert eq() == L.MBK_OK and not (rgba == 0xA5).all()
    rgba[:] = 0xA5

    # histograms
    def histogram(v=cv, c=(-0.8, 0.156), m=mrd, flags=0, dst=hist, launch_form=False):
        if launch_form:
            return lib.mbk_julia_view_histogram_launch(gpu._h, C.byref(v), c[0], c[1], m, flags, d_h.data_ptr(), None)
        return lib.mbk_julia_view_histogram_compute(gpu._h, C.byref(v) if v is not None else None, c[0], c[1], m, flags,
                                                    dst.ctypes.data if dst is not None else None, None)

    hist_cases = {
        "mrd 0": dict(m=0), "mrd above the limit": dict(m=L.MBK_HISTOGRAM_MAX_MRD + 1), "scan": dict(flags=L.MBK_KERNEL_SCAN),
        "refill": dict(flags=L.MBK_KERNEL_REFILL), "fp32": dict(flags=L.MBK_PRECISION_F32), "an output flag": dict(flags=L.MBK_WANT_BYTES),
        "lazy uniform": dict(flags=L.MBK_LAZY_UNIFORM), "c NaN": dict(c=(np.nan, np.nan)),
        "empty window": dict(v=gpu._cview(view, (0, 0, 64, 0))),
    }
    for name, kw in hist_cases.items():
        assert histogram(**kw) == bad and untouched(), name
        assert histogram(launch_form=True, **kw) == bad, name
    assert histogram(v=None) == bad and histogram(dst=None) == bad and untouched()

    torch.cuda.synchronize()
    assert (d_c == -7).all() and (d_b == 0xA5).all() and (d_s == -7.0).all() and (d_h == 12345).all() and (d_i == 0xA5).all()
    # and the context still works
    got = gpu.compute_julia_view(view, (-0.8, 0.156), mrd, want_bytes=False)[0]
    assert np.array_equal(got, J.julia_view((-1.7, -1.3, 3.4, 2.6, 64, 48), (-0.8, 0.156), mrd)[0])
