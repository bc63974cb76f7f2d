"""Small windows at extreme positions of views of up to 2^32 - 1 samples per axis, and windows on either side of every geometric
threshold of the launch path (csrc/mbk_api.hip block_launch_plan, launch_scan_t) -- run with -m gpu.

(a) The far corner (both pinned samples, ragged: the padded lanes' view indices pass 2^32 where the axis has 2^32 - 1 samples),
a window over index 2^31, the first block, and whole blocks that end one column before the view does.  The views are placed
(geometry_model.place_view) so that each window lies on the set's boundary in the seahorse valley at a pixel step of 7e-10; the
reference is tests/geometry_model.py -- one axis sample at a time, no whole axis -- and each family's own numpy model on the
window's pixels.  Every launch writes into a torch buffer between two 4 KiB guards of 0xA5.

(b) One window on each side of 16 384 blocks, of 0xffff block rows and workgroup columns, of the units kernel's widths, of the
row strips' 512 columns, of the XCD map's multiple of 32 and of the scan path's byte-stride guard; each test derives the
block counts from its window and asserts which side it is on.  These views are small enough for the C oracle."""
import numpy as np
import pytest

import distance_model as DM
import geometry_model as G
import julia_model as J
import render_model as RM
import smooth_truth as T
from distributedmandelbrot_amd import MbkError, Palette, View

pytestmark = pytest.mark.gpu

ANCHOR = (-0.7412314824132358, 0.11228268942084964)     # chaotic at this scale: counts from ~1300 up and pixels that stay
INSIDE = (-0.1, 0.1)                                     # inside the main cardioid
STEP = 7e-10
MRD = 5000
SIZES = [(2 ** 31 - 1, 2 ** 32 - 1), (2 ** 31, 2 ** 31 + 9), (2 ** 31 + 9, 2 ** 31), (2 ** 32 - 1, 2 ** 31 - 1)]
KERNELS = ["default", "simple", "asm", "refill", "group", "scan"]
GUARD = 4096


def windows(w, h):
    """The four windows of (a).  `around_2^31` starts at index 2^31 - 5 and is 21 wide on every axis that holds index 2^31 + 15;
    an axis of 2^31 - 1 or 2^31 samples cannot, and there the window is the axis' 21 samples that end three short of its end (up
    to index 2^31 - 5 or - 4: the largest indices a signed conversion still gets right).  SIZES gives each axis both kinds:
    index 2^31 is crossed by the columns of two of the four views and by the rows of the other two.  `before_the_edge` ends at column w - 2
    and row h - 2 and starts off the 8-grid; where w - 73 is a multiple of 8 it is 75 columns wide instead of 72."""
    ncols = 72 if (w - 73) % 8 else 75
    out = {"far_corner": (w - 13, h - 11, 13, 11),
           "around_2^31": (min(2 ** 31 - 5, w - 24), min(2 ** 31 - 5, h - 24), 21, 21),
           "first_block": (0, 0, 8, 8),
           "before_the_edge": (w - 1 - ncols, h - 41, ncols, 40)}
    assert out["before_the_edge"][0] % 8 != 0 and out["before_the_edge"][0] + ncols - 1 == w - 2
    return out


CASES = [(w, h, name) for w, h in SIZES for name in ("far_corner", "around_2^31", "first_block", "before_the_edge")]
CASE_IDS = [f"{w}x{h}-{name}" for w, h, name in CASES]


def case_view(w, h, name, anchor=ANCHOR):
    window = windows(w, h)[name]
    return G.place_view(anchor, STEP, w, h, window), window


class Guarded:
    """n elements of `dtype` on the device between two 4 KiB guards of 0xA5; the body starts as 0xA5 too."""

    def __init__(self, dtype, n):
        import torch
        self.dtype, self.n = np.dtype(dtype), int(n)
        self.nbytes = self.n * self.dtype.itemsize
        self.t = torch.full((2 * GUARD + (self.nbytes + 7) // 8 * 8,), 0xA5, dtype=torch.uint8, device="cuda:0")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def zero(self):
        self.t[GUARD:GUARD + self.nbytes].zero_()
        return self

    def get(self, shape=None):
        """The body on the host; asserts that both guards are what they were."""
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + self.nbytes:] == 0xA5).all(), "a guard was written"
        body = h[GUARD:GUARD + self.nbytes].view(self.dtype)
        return body.reshape(shape) if shape is not None else body


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sync():
    import torch
    torch.cuda.synchronize()


def launch_plain(dev, view, window, mrd, kernel, precision="f64", counts=True, byts=True):
    shape = (window[3], window[2])
    n = shape[0] * shape[1]
    dc, db = (Guarded(np.int32, n) if counts else None), (Guarded(np.uint8, n) if byts else None)
    _sync()
    dev.launch_view(View(*view), mrd, d_counts=dc.ptr if counts else 0, d_bytes=db.ptr if byts else 0, stream=_stream(), window=window,
                    kernel=kernel, precision=precision)
    _sync()
    return (dc.get(shape) if counts else None), (db.get(shape) if byts else None)


_REF = {}


def reference(view, window, mrd=MRD, precision="f64"):
    key = (view, window, mrd, precision)
    if key not in _REF:
        _REF[key] = G.window_counts(view, window, mrd, precision)
    return _REF[key]


def assert_variety(counts, what):
    assert len(np.unique(counts)) >= 20 and (counts == 0).any() and (counts > 0).any(), (what, len(np.unique(counts)))


@pytest.fixture(scope="module")
def strict():
    """A second ctx with the cycle test off."""
    from distributedmandelbrot_amd import MandelbrotDevice
    with MandelbrotDevice(0) as dev:
        dev.set_option("cycle_detect", 0)
        yield dev


# ---- (a) plain views ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,name", CASES, ids=CASE_IDS)
def test_plain_counts_and_bytes_through_every_selector(gpu, strict, w, h, name):
    view, window = case_view(w, h, name)
    oc, ob = reference(view, window)
    assert_variety(oc, (w, h, name))
    for dev, cyc in ((gpu, 1), (strict, 0)):
        assert dev.get_option("cycle_detect") == cyc
        for kernel in KERNELS:
            c, b = launch_plain(dev, view, window, MRD, kernel)
            assert np.array_equal(c, oc), (w, h, name, kernel, cyc, int((c != oc).sum()))
            assert np.array_equal(b, ob), (w, h, name, kernel, cyc)
    # one output alone (other kernel instantiations), and the synchronous form with its statistics
    c, _ = launch_plain(gpu, view, window, MRD, "scan", byts=False)
    _, b = launch_plain(gpu, view, window, MRD, "group", counts=False)
    assert np.array_equal(c, oc) and np.array_equal(b, ob), (w, h, name)
    c, b, st = gpu.compute_view(View(*view), MRD, window=window)
    assert np.array_equal(c, oc) and np.array_equal(b, ob)
    assert st.never_pixels == int((oc == 0).sum()) and st.pixel_iterations == int(np.where(oc > 0, oc, MRD - 1).astype(np.int64).sum())


@pytest.mark.parametrize("w,h,name", CASES, ids=CASE_IDS)
def test_plain_fp32(gpu, strict, w, h, name):
    """The coordinates are generated in binary64 and rounded once: at this step binary32 sees a handful of distinct points, which
    the reference reproduces (numpy_escape in float32 on the same samples)."""
    view, window = case_view(w, h, name)
    oc, ob = reference(view, window, 600, "f32")
    for dev in (gpu, strict):
        for kernel in ("asm", "group"):
            c, b = launch_plain(dev, view, window, 600, kernel, precision="f32")
            assert np.array_equal(c, oc), (w, h, name, kernel, int((c != oc).sum()))
            assert np.array_equal(b, ob), (w, h, name, kernel)


@pytest.mark.parametrize("w,h,name", CASES, ids=CASE_IDS)
def test_plain_smooth(gpu, w, h, name):
    view, window = case_view(w, h, name)
    oc, mag = G.window_escape(view, window, MRD)
    assert np.array_equal(oc, reference(view, window)[0])
    assert_variety(oc, (w, h, name))
    n = oc.size
    for kernel in ("default", "asm", "group", "scan"):
        ds, dc = Guarded(np.float64, n), Guarded(np.int32, n)
        _sync()
        gpu.launch_view_smooth(View(*view), MRD, d_smooth=ds.ptr, d_counts=dc.ptr, stream=_stream(), window=window, kernel=kernel)
        _sync()
        assert np.array_equal(dc.get(oc.shape), oc), (w, h, name, kernel)
        T.assert_within(ds.get(oc.shape), oc, mag, f"{w}x{h} {name} {kernel}")


@pytest.mark.parametrize("w,h", SIZES)
def test_sure_interior_forced_at_the_far_edge(strict, w, h):
    """MBK_OPT_SURE_INTERIOR = 2 on whole blocks that end one column before the view does: inside the cardioid every block's
    constant stores go through the scalar base fetched from the kernel arguments; on the boundary every block trips the final test
    and is computed again."""
    saved = strict.get_option("sure_interior")
    try:
        for anchor, mrd in ((INSIDE, 200), (ANCHOR, MRD)):
            view, window = case_view(w, h, "before_the_edge", anchor)
            oc, ob = reference(view, window, mrd)
            assert (not oc.any()) if anchor == INSIDE else ((oc > 0).any() and (oc == 0).any())
            for option in (2, 0):
                strict.set_option("sure_interior", option)
                for kernel in ("group", "asm"):
                    c, b = launch_plain(strict, view, window, mrd, kernel)
                    assert np.array_equal(c, oc) and np.array_equal(b, ob), (w, h, anchor, option, kernel)
                ds, dc = Guarded(np.float64, oc.size), Guarded(np.int32, oc.size)
                _sync()
                strict.launch_view_smooth(View(*view), mrd, d_smooth=ds.ptr, d_counts=dc.ptr, stream=_stream(), window=window, kernel="group")
                _sync()
                assert np.array_equal(dc.get(oc.shape), oc) and np.array_equal(ds.get(oc.shape) == 0.0, oc == 0), (w, h, anchor, option)
    finally:
        strict.set_option("sure_interior", saved)


# ---- (a) the two-pass families, Julia views, the histogram -------------------------------------------------------------------------

EDGE_CASES = [(w, h, name) for w, h in SIZES for name in ("far_corner", "around_2^31")]
EDGE_IDS = [f"{w}x{h}-{name}" for w, h, name in EDGE_CASES]


@pytest.mark.parametrize("w,h,name", EDGE_CASES, ids=EDGE_IDS)
def test_distance(gpu, w, h, name):
    """Held to tests/distance_model.py as tests/test_gpu_distance.py holds the small views: the counts bit for bit, the final
    state by assert_states_agree, the expression within D_GPU."""
    view, window = case_view(w, h, name)
    mrd = 3000
    cr, ci = G.view_window(view, window)
    st = DM.states(cr.ravel(), ci.ravel(), mrd)
    mn = st["n"].reshape(cr.shape)
    assert np.array_equal(mn, reference(view, window, mrd)[0]) and (mn > 0).any() and (mn == 0).any()
    for kernel in ("default", "asm", "group", "scan"):
        dd, dc = Guarded(np.float64, mn.size), Guarded(np.int32, mn.size)
        _sync()
        gpu.launch_view_distance(View(*view), mrd, d_distance=dd.ptr, d_counts=dc.ptr, stream=_stream(), window=window, kernel=kernel)
        _sync()
        de, c = dd.get(mn.shape), dc.get(mn.shape)
        what = f"{w}x{h} {name} {kernel}"
        assert np.array_equal(c, mn), (what, int((c != mn).sum()))
        assert not np.isnan(de).any() and (de[c == 0] == 0.0).all() and (de >= 0.0).all(), what
        DM.assert_states_agree(de, st, what)
        DM.assert_expression_within(de, st, what, DM.D_GPU)


@pytest.mark.parametrize("w,h,name", EDGE_CASES, ids=EDGE_IDS)
def test_julia_counts_bytes_and_smooth(gpu, w, h, name):
    """The Julia set of the anchor itself: the pixel at the anchor runs the Mandelbrot orbit of a boundary point, so the window lies
    on this Julia set's boundary.  Held to tests/julia_model.py as tests/test_gpu_julia.py does."""
    view, window = case_view(w, h, name)
    mrd = 3000
    cr, ci = G.view_window(view, window)
    wn, wmag = J.julia_counts(cr, ci, ANCHOR[0], ANCHOR[1], mrd)
    assert len(np.unique(wn)) >= 20, len(np.unique(wn))
    for kernel in ("default", "asm", "group"):
        dc, db, ds = Guarded(np.int32, wn.size), Guarded(np.uint8, wn.size), Guarded(np.float64, wn.size)
        _sync()
        gpu.launch_julia_view(View(*view), ANCHOR, mrd, d_counts=dc.ptr, d_bytes=db.ptr, d_smooth=ds.ptr, stream=_stream(), window=window,
                              kernel=kernel)
        _sync()
        what = f"{w}x{h} {name} {kernel}"
        c = dc.get(wn.shape)
        assert np.array_equal(c, wn), (what, int((c != wn).sum()))
        assert np.array_equal(db.get(wn.shape), J.quantise(wn, mrd)), what
        T.assert_within(ds.get(wn.shape), wn, wmag, what)


@pytest.mark.parametrize("w,h,name", EDGE_CASES, ids=EDGE_IDS)
def test_view_histogram_launch(gpu, w, h, name):
    view, window = case_view(w, h, name)
    oc, _ = reference(view, window)
    hist = Guarded(np.int64, MRD).zero()
    _sync()
    gpu.launch_view_histogram(View(*view), MRD, d_hist=hist.ptr, stream=_stream(), window=window)
    _sync()
    assert np.array_equal(hist.get(), np.bincount(oc.ravel(), minlength=MRD).astype(np.int64)), (w, h, name)


# ---- (a) renders: W * s up to 2^32 - 2 ----------------------------------------------------------------------------------------------

RENDER_PAL = Palette(np.random.RandomState(1).randint(0, 256, (256, 4)).astype(np.uint8))
SMOOTH_PAL = Palette.cosine(1000, period=7.3, inside=(10, 20, 30, 255))


@pytest.mark.parametrize("w", [2 ** 31 - 1, 2 ** 31 - 2])
@pytest.mark.parametrize("rows", [0, 5])
def test_renders_at_the_largest_supersampled_width(gpu, w, rows):
    """Supersample 2 of a view 2^31 - 1 (2^31 - 2) wide and high: the finer view has 2^32 - 2 (2^32 - 4) samples per axis, the most
    the check accepts.  The far corner, in one band and in bands of 5 rows.  The bytes image is the model's on the reference's
    bytes of the finer view's window; the smooth image is the model's on the device's own samples of that window, whose counts are
    held to the reference and whose values to the correctly rounded formula on the reference's |z|^2 (smooth_truth) here."""
    s, h = 2, w
    window = (w - 13, h - 11, 13, 11)
    fine_window = tuple(s * x for x in window)
    view = G.place_view(ANCHOR, STEP, w, h, window)
    fine = (view[0], view[1], view[2], view[3], w * s, h * s)
    assert fine[4] == (2 ** 32 - 2 if w == 2 ** 31 - 1 else 2 ** 32 - 4)
    oc, ob = reference(fine, fine_window, 3000)
    assert_variety(oc, ("render", w))
    n = window[2] * window[3]
    out = Guarded(np.uint8, 4 * n)
    _sync()
    gpu.launch_render_view(View(*view), 3000, palette=RENDER_PAL, d_rgba=out.ptr, source="bytes", supersample=s, window=window,
                           max_band_rows=rows, stream=_stream())
    _sync()
    want = RM.render_bytes(RENDER_PAL.entries, s, ob)
    got = out.get((window[3], window[2], 4))
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())
    nu, counts, _ = gpu.compute_view_smooth(View(*fine), 3000, window=fine_window)
    rc, mag = G.window_escape(fine, fine_window, 3000)
    assert np.array_equal(counts, oc) and np.array_equal(rc, oc)
    T.assert_within(nu, rc, mag, f"render samples, width {w}")
    out = Guarded(np.uint8, 4 * n)
    _sync()
    gpu.launch_render_view(View(*view), 3000, palette=SMOOTH_PAL, d_rgba=out.ptr, source="smooth", supersample=s, window=window,
                           max_band_rows=rows, stream=_stream())
    _sync()
    want = RM.render_smooth(SMOOTH_PAL.entries, SMOOTH_PAL.inside, SMOOTH_PAL.scale, SMOOTH_PAL.offset, s, counts, nu)
    got = out.get((window[3], window[2], 4))
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())


def test_a_render_whose_finer_view_has_2_to_the_32_samples_is_refused(gpu):
    w = 2 ** 31
    window = (w - 13, w - 11, 13, 11)
    view = G.place_view(ANCHOR, STEP, w, w, window)
    out = Guarded(np.uint8, 4 * 13 * 11)
    for source, pal in (("bytes", RENDER_PAL), ("smooth", SMOOTH_PAL)):
        with pytest.raises(MbkError):
            gpu.launch_render_view(View(*view), 100, palette=pal, d_rgba=out.ptr, source=source, supersample=2, window=window, stream=_stream())
    _sync()
    assert (out.get() == 0xA5).all()


# ---- (b) threshold shapes ------------------------------------------------------------------------------------------------------------

FULL = (-2.0, -1.5, 3.0, 3.0)
STRIP = (-0.7501, -1.2, 0.0002, 2.3)          # a thin strip across the set at x = -0.75
BAND = (-2.0, 0.049, 3.0, 0.002)              # a flat band across the set at y = 0.05
EXTERIOR = (-2.0, -2.0, 1.0, 1.0)             # no probe pixel outlives the light pass: "scan" finishes in place
BELOW = (-2.0, -2.0, 4.0, 0.9)                # the same, with counts from 1 to 8 and more (tests/test_gpu_parity.py STRIP_VIEWS)


def _check(oracle, gpu, area, ncols, nrows, mrd, kernel, options, outputs=("counts", "bytes")):
    """A view of ncols x nrows over `area` under `options` (put back afterwards), through launch_view, against the C oracle."""
    view = area + (ncols, nrows)
    key = ("oracle", view, mrd)
    if key not in _REF:
        _REF[key] = oracle.view(*view, mrd)[:2]
    oc, ob = _REF[key]
    saved = {k: gpu.get_option(k) for k in options}
    try:
        for k, v in options.items():
            gpu.set_option(k, v)
        c, b = launch_plain(gpu, view, (0, 0, ncols, nrows), mrd, kernel, counts="counts" in outputs, byts="bytes" in outputs)
    finally:
        for k, v in saved.items():
            gpu.set_option(k, v)
    if "counts" in outputs:
        assert np.array_equal(c, oc), (view, kernel, options, int((c != oc).sum()))
    if "bytes" in outputs:
        assert np.array_equal(b, ob), (view, kernel, options)
    return oc


def _blocks(ncols, nrows):
    return (ncols + 7) // 8, (nrows + 7) // 8


@pytest.mark.parametrize("ncols,nrows,side", [(1032, 1016, "below"), (1024, 1024, "at")])
def test_grid_of_16384_blocks(gpu, oracle, ncols, nrows, side):
    """grid >= 16384: a dispatch list (order 2), the units kernel (order 3), "scan" for the default selector; one block fewer: one
    kernel in image order for all of them."""
    bx, by = _blocks(ncols, nrows)
    assert bx * by == (16383 if side == "below" else 16384)
    assert gpu.get_option("waves_per_wg") == 1 and 100 > 2 * gpu.get_option("probe_steps")
    for kernel, options in (("group", {"order": 2}), ("group", {"order": 3, "units_min_light": 0}), ("default", {"heavy_share": 65536}),
                            ("default", {"heavy_share": 0})):
        oc = _check(oracle, gpu, FULL, ncols, nrows, 100, kernel, options)
    assert (oc == 0).any() and len(np.unique(oc)) > 20


@pytest.mark.parametrize("by", [65535, 65536, 65537])
def test_block_rows_around_0xffff(gpu, oracle, by):
    """A dispatch list packs the block row into 16 bits: 65 535 block rows is the most a list serves, one more goes in image order.
    8 columns: one block per row."""
    ncols, nrows = 8, 8 * by
    assert _blocks(ncols, nrows) == (1, by) and by >= 16384 and (by <= 0xffff) == (by == 65535)
    for options in ({"order": 2}, {"order": 3}, {"order": 0}):
        oc = _check(oracle, gpu, STRIP, ncols, nrows, 100, "group", options)
    _check(oracle, gpu, STRIP, ncols, nrows, 100, "default", {"heavy_share": 65536})
    assert (oc == 0).any() and len(np.unique(oc)) > 20


@pytest.mark.parametrize("by", [65535, 65536])
def test_block_rows_around_0xffff_under_the_units_kernel(gpu, oracle, by):
    """64 columns are eight block columns, one unit: the units kernel serves 65 535 block rows and leaves 65 536 to image order."""
    ncols, nrows = 64, 8 * by
    bx, nby = _blocks(ncols, nrows)
    assert (bx, nby) == (8, by) and bx % 8 == 0 and bx * nby >= 16384
    _check(oracle, gpu, STRIP, ncols, nrows, 64, "group", {"order": 3, "units_min_light": 0})


@pytest.mark.parametrize("bx", [65535, 65536, 65537])
def test_workgroup_columns_around_0xffff(gpu, oracle, bx):
    """... and the workgroup column into the other 16.  Both conditions count blocks, so they are conservative by one: 65 536 rows or
    columns have indices up to 65 535 and would still fit.  65 537 is the first width (and, above, the first height) whose last
    index does not: the case that fails if a condition lets it through to a list.  The scan selector falls back to "group" here:
    65 535 block columns are more than any resident grid (blocks_x > wmax)."""
    ncols, nrows = 8 * bx, 8
    assert _blocks(ncols, nrows) == (bx, 1) and bx >= 16384 and (bx <= 0xffff) == (bx == 65535)
    occ = gpu.scan_occupancy()
    assert bx > gpu.info()["compute_units"] * max(occ.values())
    for kernel, options in (("group", {"order": 2}), ("group", {"order": 3}), ("scan", {}), ("asm", {"order": 2})):
        oc = _check(oracle, gpu, BAND, ncols, nrows, 100, kernel, options)
    assert (oc == 0).any() and len(np.unique(oc)) > 20


@pytest.mark.parametrize("bx", [2040, 2048, 2049, 2056])
def test_units_kernel_widths(gpu, oracle, bx):
    """The units kernel serves widths of whole units (blocks_x % 8 == 0) up to 2048 block columns."""
    ncols, nrows = 8 * bx - (3 if bx % 8 else 0), 72
    assert _blocks(ncols, nrows) == (bx, 9) and bx * 9 >= 16384
    served = bx % 8 == 0 and bx <= 2048
    assert served == (bx in (2040, 2048))
    for outputs in (("counts", "bytes"), ("bytes",)):
        oc = _check(oracle, gpu, BAND, ncols, nrows, 100, "group", {"order": 3, "units_min_light": 0}, outputs)
    assert (oc == 0).any() and len(np.unique(oc)) > 20


@pytest.mark.parametrize("ncols", [511, 512])
def test_row_strips_from_512_columns(gpu, oracle, ncols):
    for options in ({"scan_strip": 1, "scan_inline": 1}, {"scan_strip": 0, "scan_inline": 1}):
        for outputs in (("counts", "bytes"), ("bytes",), ("counts",)):
            oc = _check(oracle, gpu, BELOW, ncols, 67, 100, "scan", options, outputs)
    assert len(np.unique(oc)) >= 6


@pytest.mark.parametrize("ncols", [1024, 1088])
def test_xcd_map_needs_a_multiple_of_32_block_columns(gpu, oracle, ncols):
    bx, _ = _blocks(ncols, 128)
    assert bx % 32 == (0 if ncols == 1024 else 8)
    for options in ({"scan_xcd_map": 1}, {"scan_xcd_map": 0}, {"scan_xcd_map": 1, "scan_inline": 0}):
        oc = _check(oracle, gpu, FULL, ncols, 128, 100, "scan", options)
    assert (oc == 0).any() and len(np.unique(oc)) > 20
    _check(oracle, gpu, EXTERIOR, ncols, 128, 100, "scan", {"scan_xcd_map": 1, "scan_strip": 0})


@pytest.mark.parametrize("narrower", [0, 8])
def test_byte_stride_guard_width(gpu, narrower):
    """launch_scan_t leaves a window to "group" when stride_by * region_h * out_pitch * 4 >= 2^31.  With 8 rows stride_by * region_h is
    at most 8 (eight 1-row strips, or one 8-row block), so the narrowest window that trips the guard has 2^31 / 32 columns.  At that
    width the launch never reaches the guard: blocks_x = 2^23 exceeds every resident grid and the check before it (blocks_x > wmax)
    has sent it to "group" already -- and a width that passes that check keeps the product far below 2^31 (asserted below from
    the device's own occupancy).  So the guard is unreachable through the C ABI.  Both widths are computed all the same, bytes
    only.  2^29 pixels are too many for a CPU reference within a test's seconds: the bytes are compared on the device with the same
    window computed in eight bands through "asm", and 4 224 of its columns -- both ends, seeded ones -- with the numpy reference."""
    import torch
    from oracle.oracle import numpy_escape, numpy_quantise
    full = next(n for n in range(2 ** 26 - 64, 2 ** 26 + 64, 8) if 8 * 1 * n * 4 >= 2 ** 31)
    ncols, nrows, mrd = full - narrower, 8, 16
    assert (8 * ncols * 4 >= 2 ** 31) == (narrower == 0) and ncols * nrows <= 2 ** 31
    wmax = gpu.info()["compute_units"] * max(gpu.scan_occupancy().values())
    assert _blocks(ncols, nrows)[0] > wmax
    # any window the scan path does serve: stride_by * regions_x <= wmax, a region is at most 64 columns wide and 8 rows high
    assert wmax * 64 * 8 * 4 < 2 ** 31
    view = BAND + (full, nrows)
    out = Guarded(np.uint8, ncols * nrows)
    _sync()
    gpu.launch_view(View(*view), mrd, d_bytes=out.ptr, stream=_stream(), window=(0, 0, ncols, nrows), kernel="scan")
    _sync()
    body = out.t[GUARD:GUARD + ncols * nrows].view(nrows, ncols)
    assert bool((out.t[:GUARD] == 0xA5).all()) and bool((out.t[GUARD + ncols * nrows:] == 0xA5).all()), "a guard was written"
    band = Guarded(np.uint8, 2 ** 26)
    for c0 in range(0, ncols, 2 ** 23):
        nc = min(2 ** 23, ncols - c0)
        gpu.launch_view(View(*view), mrd, d_bytes=band.ptr, stream=_stream(), window=(c0, 0, nc, nrows), kernel="asm")
        _sync()
        assert torch.equal(band.t[GUARD:GUARD + nc * nrows].view(nrows, nc), body[:, c0:c0 + nc]), (narrower, c0)
    rs = np.random.RandomState(7)
    cols = np.unique(np.concatenate([np.arange(64), np.arange(ncols - 64, ncols), rs.randint(0, ncols, 4096)])).astype(np.uint64)
    xr = G.axis_sample(view[0], view[2], full, cols)
    xi = G.axis_sample(view[1], view[3], nrows, np.arange(nrows, dtype=np.uint64))
    want = numpy_quantise(numpy_escape(xr[None, :], xi[:, None], mrd).reshape(nrows, cols.size), mrd)
    assert len(np.unique(want)) >= 8
    got = body[:, torch.from_numpy(cols.astype(np.int64)).to("cuda:0")].cpu().numpy()
    assert np.array_equal(got, want)


# ---- (a) deep views: pixel offsets (k - (W - 1) / 2) * s at k up to 2^32 - 2 ---------------------------------------------------------

DEEP_STEP = 1e-12


def deep_windows(w, h):
    return {"far_corner": (w - 13, h - 11, 13, 11), "around_2^31": (min(2 ** 31 - 5, w - 24), 2 ** 31 - 5, 21, 21), "first_block": (0, 0, 8, 8),
            "centre": ((w - 1) // 2 - 6, (h - 1) // 2 - 4, 13, 11)}


def deep_case(w, name, mrd):
    """(orbit, view, window) of a w x (2^32 - 2) deep view of pixel step 1e-12 whose window `name` has its first pixel at ANCHOR:
    the orbit's centre is ANCHOR minus that pixel's offset, exactly (rationals).  The even height makes the centre offset
    (h - 1) / 2 a half-integer; offsets reach 2e-3."""
    import deep_model as D
    from fractions import Fraction
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    h = 2 ** 32 - 2
    view = DeepView(DEEP_STEP * (w - 1), w, h, DEEP_STEP * (h - 1))
    window = deep_windows(w, h)[name]
    dr, di = D.offsets(view, window)
    orbit = DeepOrbit(Fraction(ANCHOR[0]) - Fraction(float(dr[0])), Fraction(ANCHOR[1]) - Fraction(float(di[0])), mrd, min_span=DEEP_STEP)
    return orbit, view, window


@pytest.mark.parametrize("name", ["far_corner", "around_2^31", "first_block", "centre"])
@pytest.mark.parametrize("w", [2 ** 31 - 1, 2 ** 32 - 1])
def test_deep_view_counts_and_distance(gpu, w, name):
    """A deep view's pixel offset is (k - (W - 1) / 2) * s: a half-integer times s where W is even, and k is up to 2^32 - 2.  Counts
    (plain step and BLA) bit for bit against tests/deep_model.py through offsets(view, window) on the library's own orbit table (as
    tests/test_gpu_deep.py), the distance estimate against tests/deep_distance_model.py as tests/test_gpu_deep_distance.py holds
    it.  Each window holds at least 20 distinct counts and pixels that stay: half a pixel of error in an offset moves counts."""
    import deep_distance_model as DD
    import deep_model as D
    mrd = 3000
    orbit, view, window = deep_case(w, name, mrd)
    zr, zi = orbit.table()
    dr, di = D.offsets(view, window)
    want, _ = D.model_counts(zr, zi, dr, di, mrd)
    want = want.reshape(window[3], window[2])
    assert_variety(want, (w, name))
    for bla in (False, True):
        dc = Guarded(np.int32, want.size)
        _sync()
        gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.ptr, stream=_stream(), window=window, bla=bla)
        _sync()
        got = dc.get(want.shape)
        assert np.array_equal(got, want), (w, window, bla, int((got != want).sum()))
    st = DD.states(zr, zi, dr, di, mrd)
    assert np.array_equal(st["n"].reshape(want.shape), want)
    drel, dc = Guarded(np.float64, want.size), Guarded(np.int32, want.size)
    _sync()
    gpu.launch_deep_view_distance(orbit, view, mrd, d_rel=drel.ptr, d_counts=dc.ptr, stream=_stream(), window=window)
    _sync()
    rel = drel.get(want.shape)
    assert np.array_equal(dc.get(want.shape), want)
    assert not np.isnan(rel).any() and (rel[want == 0] == 0.0).all() and (rel >= 0.0).all()
    DD.assert_states_agree(rel, st, view.span_r, f"deep distance {w} {name}")


# ---- (a) normals, relief renders, interior values, Julia distance, density, adaptive renders -----------------------------------------

@pytest.mark.parametrize("w,h,name", EDGE_CASES, ids=EDGE_IDS)
def test_normals_and_relief_render(gpu, w, h, name):
    """Normals and their distance bit for bit against tests/relief_model.py on the window's pixels (as tests/test_gpu_relief.py);
    the relief render at supersample 1 against the model's image of the device's smooth values and the model's normals."""
    import math
    import relief_model as RM
    view, window = case_view(w, h, name)
    mrd = 3000
    cr, ci = G.view_window(view, window)
    st = DM.states(cr.ravel(), ci.ravel(), mrd)
    mn = st["n"].reshape(cr.shape)
    want = RM.normal(st["zr"], st["zi"], st["dr"], st["di"], st["n"]).reshape(cr.shape + (2,))
    assert (mn > 0).any() and (mn == 0).any() and (want[mn > 0] != 0.0).any(axis=1).all()
    for kernel in ("default", "asm"):
        dn, dc, dd = Guarded(np.float64, 2 * mn.size), Guarded(np.int32, mn.size), Guarded(np.float64, mn.size)
        _sync()
        gpu.launch_view_normals(View(*view), mrd, d_normals=dn.ptr, d_counts=dc.ptr, d_distance=dd.ptr, stream=_stream(), window=window,
                                kernel=kernel)
        _sync()
        assert np.array_equal(dc.get(mn.shape), mn), (w, h, name, kernel)
        got = dn.get(want.shape)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (w, h, name, kernel, int((got != want).any(axis=2).sum()))
        de = dd.get(mn.shape)
        DM.assert_states_agree(de, st, f"normals' distance {w}x{h} {name} {kernel}")
    nu = Guarded(np.float64, mn.size)
    _sync()
    gpu.launch_view_smooth(View(*view), mrd, d_smooth=nu.ptr, stream=_stream(), window=window)
    _sync()
    light, height = (math.cos(0.6), math.sin(0.6)), 1.25
    for rows in (0, 5):
        out = Guarded(np.uint8, 4 * mn.size)
        _sync()
        gpu.launch_render_view_relief(View(*view), mrd, palette=SMOOTH_PAL, d_rgba=out.ptr, light=light, height=height, supersample=1,
                                      window=window, max_band_rows=rows, stream=_stream())
        _sync()
        model = RM.render(SMOOTH_PAL.entries, SMOOTH_PAL.inside, SMOOTH_PAL.scale, SMOOTH_PAL.offset, light[0], light[1], height, 1, mn,
                          nu.get(mn.shape), want)
        img = out.get(mn.shape + (4,))
        assert np.array_equal(img, model), (w, h, name, rows, int((img != model).any(axis=2).sum()))


@pytest.mark.parametrize("w,h,name", EDGE_CASES, ids=EDGE_IDS)
def test_interior_values(gpu, w, h, name):
    """Periods and interior distance estimates bit for bit against tests/interior_model.py (as tests/test_gpu_interior.py).  At a
    step of 7e-10 nothing beside the boundary settles or escapes within a test's mrd, so these views have a pixel step of 0.02
    (their extent is 4e7 and more, far inside what validate_view accepts): the windows lie over the top of the main cardioid
    and hold settled pixels of several periods, pixels that run to the end and exterior ones."""
    import interior_model as IM
    window = windows(w, h)[name]
    view = G.place_view((-0.3, 0.5), 0.02, w, h, window)
    mrd = 600
    cr, ci = G.view_window(view, window)
    m = {k: a.reshape(cr.shape) for k, a in IM.interior(cr, ci, mrd).items()}
    for kernel in ("default", "scan", "group"):
        dp, dd, dc = Guarded(np.int32, cr.size), Guarded(np.float64, cr.size), Guarded(np.int32, cr.size)
        _sync()
        gpu.launch_view_interior(View(*view), mrd, d_period=dp.ptr, d_distance=dd.ptr, d_counts=dc.ptr, stream=_stream(), window=window,
                                 kernel=kernel)
        _sync()
        what = (w, h, name, kernel)
        assert np.array_equal(dc.get(cr.shape), m["n"]), what
        assert np.array_equal(dp.get(cr.shape), m["period"]), what
        assert np.array_equal(dd.get(cr.shape).view(np.uint64), m["de"].view(np.uint64)), what
    assert (m["n"] > 0).any() and len(np.unique(m["period"])) >= 3 and (m["de"] > 0.0).sum() >= 50


@pytest.mark.parametrize("w,h,name", EDGE_CASES, ids=EDGE_IDS)
def test_julia_distance(gpu, w, h, name):
    """Held to tests/julia_distance_model.py as tests/test_gpu_julia_distance.py holds the small views."""
    import julia_distance_model as JM
    view, window = case_view(w, h, name)
    mrd = 3000
    cr, ci = G.view_window(view, window)
    st = JM.states(cr.ravel(), ci.ravel(), ANCHOR, mrd)
    mn = st["n"].reshape(cr.shape)
    assert len(np.unique(mn)) >= 20
    for kernel in ("default", "asm", "group"):
        dd, dc = Guarded(np.float64, mn.size), Guarded(np.int32, mn.size)
        _sync()
        gpu.launch_julia_view_distance(View(*view), ANCHOR, mrd, d_distance=dd.ptr, d_counts=dc.ptr, stream=_stream(), window=window,
                                       kernel=kernel)
        _sync()
        what = f"julia distance {w}x{h} {name} {kernel}"
        de, n = dd.get(mn.shape), dc.get(mn.shape)
        assert np.array_equal(n, mn), (what, int((n != mn).sum()))
        assert not np.isnan(de).any() and np.array_equal(de == 0.0, n == 0) and (de >= 0.0).all(), what
        JM.assert_states_agree(de, st, what)
        JM.assert_expression_within(de, st, what, JM.J_GPU)


@pytest.mark.parametrize("w,h", SIZES)
def test_density_from_the_far_corner_of_a_huge_sampling_view(gpu, w, h):
    """The far-corner window of a huge sampling view deposits its orbits into a small target: exactly tests/density_model.py's
    table on the window's coordinates."""
    import density_model as DEN
    from distributedmandelbrot_amd import DensityTarget
    view, window = case_view(w, h, "far_corner")
    target, mrd = DensityTarget(-2.5, -2.5, 5.0, 5.0, 64, 48), 3000
    want, deposits, _, n = DEN.accumulate(View(*view), target, mrd, window=window, coords=G.window_axes(view, window))
    assert deposits > 10000 and (n == 0).any() and len(np.unique(n)) >= 20
    table = Guarded(np.uint32, 64 * 48).zero()
    _sync()
    gpu.launch_view_density(View(*view), target, mrd, d_density=table.ptr, stream=_stream(), window=window)
    _sync()
    assert np.array_equal(table.get((48, 64)).astype(np.uint64), want)


@pytest.mark.parametrize("total", [2 ** 31 - 1, 2 ** 32 - 1])
@pytest.mark.parametrize("s", [2, 3])
def test_adaptive_render_at_its_largest_view(gpu, s, total):
    """W = H = (2^31 - 1) // s, the last view whose samples' indices fit 31 bits, and (2^32 - 1) // s, the largest the render
    check accepts (W * s <= 2^32 - 1); the far corner.  The neighbour rule at column W - 1 and row H - 1 sees neighbours
    inside the view only (adaptive_model.render_adaptive_window: the window and a one-pixel halo of the s = 1 image, clamped to the
    view).  The model runs on the device's own smooth values of the halo and of the finer view's window, whose counts are held to
    the reference and whose values to smooth_truth here.  The whole view has 2^60 pixels and more: the pixel limit of a window
    applies to the output window."""
    import adaptive_model as A
    w = h = total // s
    mrd = 3000
    window = (w - 13, h - 11, 13, 11)
    view = G.place_view(ANCHOR, STEP, w, h, window)
    fine = view[:4] + (w * s, h * s)
    hal = A.halo(window, w, h)
    assert hal == (w - 14, h - 12, 14, 12)
    samples = {}
    for key, v, win in (("halo", view, hal), ("fine", fine, tuple(s * x for x in window))):
        nu, counts, _ = gpu.compute_view_smooth(View(*v), mrd, window=win)
        rc, mag = G.window_escape(v, win, mrd)
        assert np.array_equal(counts, rc), key
        T.assert_within(nu, rc, mag, f"adaptive {key} samples s={s}")
        samples[key] = (counts, nu)
    assert_variety(samples["fine"][0], ("adaptive", s))
    masks = set()
    for thr in (0, 24, 256):
        for rows in (0, 5):
            out, dm = Guarded(np.uint8, 4 * 13 * 11), Guarded(np.uint8, 13 * 11 + 1)
            _sync()
            gpu.launch_render_view_adaptive(View(*view), mrd, palette=SMOOTH_PAL, supersample=s, threshold=thr, d_rgba=out.ptr, d_mask=dm.ptr,
                                            stream=_stream(), window=window, max_band_rows=rows)
            _sync()
            want, want_mask = A.render_adaptive_window(SMOOTH_PAL.entries, SMOOTH_PAL.inside, SMOOTH_PAL.scale, SMOOTH_PAL.offset, s, thr,
                                                       window, w, h, *samples["halo"], *samples["fine"])
            img, mask = out.get((11, 13, 4)), dm.get()[:143].reshape(11, 13)
            assert np.array_equal(mask, want_mask), (s, thr, rows)
            assert np.array_equal(img, want), (s, thr, rows, int((img != want).any(axis=2).sum()))
            masks.add((thr, int(want_mask.sum())))
    assert (0, 143) in masks and (256, 0) in masks


# ---- (a) extended-range deep views ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["far_corner", "around_2^31", "first_block", "centre"])
@pytest.mark.parametrize("w", [2 ** 31 - 1, 2 ** 32 - 1])
def test_wide_deep_view_counts(gpu, w, name):
    """The same windows of an extended-range deep view of pixel step 2^-1105 beside c = i (the "i-1100" case of
    tests/test_gpu_deep_wide.py has 2^-1104.5): the orbit's centre is i minus the offset of the window's middle pixel, exactly, so
    that every window looks at the same neighbourhood.  Plain step, bit for bit against tests/deep_wide_model.py through
    offsets(view, window) on the library's own wide table.  (XBLA is not held here: its skips round differently from the plain
    step, and its reference is the host twin of tests/test_gpu_deep_wide_bla.py, not this model.)"""
    import deep_wide_model as W
    from fractions import Fraction
    from distributedmandelbrot_amd import DeepOrbit, WideDeepView
    mrd, h = 1000, 2 ** 32 - 2
    view = WideDeepView((w - 1) / 2.0 ** 32, -1105 + 32, w, h, (h - 1) / 2.0 ** 32)
    window = deep_windows(w, h)[name]
    dr, di = W.offsets(view, window)
    k = len(dr) // 2
    unit = Fraction(2) ** view.exp2
    orbit = DeepOrbit(-Fraction(float(dr[k])) * unit, 1 - Fraction(float(di[k])) * unit, mrd, min_span_exp2=-1106)
    want, _ = W.model_counts(*orbit.wide_table(), dr, di, view.exp2, mrd)
    want = want.reshape(window[3], window[2])
    assert len(np.unique(want)) >= 5, len(np.unique(want))
    dc = Guarded(np.int32, want.size)
    _sync()
    gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.ptr, stream=_stream(), window=window)
    _sync()
    got = dc.get(want.shape)
    assert np.array_equal(got, want), (w, window, int((got != want).sum()))


# ---- (a) deep and extended-range deep views: normals, nucleus, XBLA, distance, adaptive renders --------------------------------------

def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def wide_case(w, name, mrd, h=2 ** 32 - 2, window=None):
    """(orbit, view, window) of test_wide_deep_view_counts: the window's middle pixel lies at c = i."""
    import deep_wide_model as W
    from fractions import Fraction
    from distributedmandelbrot_amd import DeepOrbit, WideDeepView
    view = WideDeepView((w - 1) / 2.0 ** 32, -1105 + 32, w, h, (h - 1) / 2.0 ** 32)
    window = window or deep_windows(w, h)[name]
    dr, di = W.offsets(view, window)
    k = len(dr) // 2
    unit = Fraction(2) ** view.exp2
    return DeepOrbit(-Fraction(float(dr[k])) * unit, 1 - Fraction(float(di[k])) * unit, mrd, min_span_exp2=-1108), view, window


DEEP_EDGE = [(w, name) for w in (2 ** 31 - 1, 2 ** 32 - 1) for name in ("far_corner", "around_2^31", "first_block", "centre")]
DEEP_EDGE_IDS = [f"{w}-{name}" for w, name in DEEP_EDGE]


@pytest.mark.parametrize("w,name", DEEP_EDGE, ids=DEEP_EDGE_IDS)
def test_deep_view_normals_and_nucleus(gpu, w, name):
    """Deep-view normals (plain step and BLA) bit for bit against tests/deep_relief_model.py, atom periods and Newton seeds bit for
    bit against tests/deep_nucleus_model.py, both through offsets(view, window), on the windows of
    test_deep_view_counts_and_distance."""
    import deep_nucleus_model as NM
    import deep_relief_model as RL
    mrd = 3000
    orbit, view, window = deep_case(w, name, mrd)
    shape = (window[3], window[2])
    n = shape[0] * shape[1]
    for bla in (False, True):
        want, mn, _, _, _ = RL.model(orbit, view, mrd, window, bla=bla)
        assert_variety(mn, (w, name, bla))
        dn, dc = Guarded(np.float64, 2 * n), Guarded(np.int32, n)
        _sync()
        gpu.launch_deep_view_normals(orbit, view, mrd, d_normals=dn.ptr, d_counts=dc.ptr, stream=_stream(), window=window, bla=bla)
        _sync()
        assert np.array_equal(dc.get(shape), mn), (w, name, bla)
        got = dn.get(shape + (2,))
        assert np.array_equal(_bits64(got), _bits64(want)), (w, name, bla, int((_bits64(got) != _bits64(want)).any(axis=2).sum()))
    st = NM.model(orbit, view, mrd, window)
    dp, dd, dc = Guarded(np.int32, n), Guarded(np.float64, 2 * n), Guarded(np.int32, n)
    _sync()
    gpu.launch_deep_view_nucleus(orbit, view, mrd, d_period=dp.ptr, d_delta=dd.ptr, d_counts=dc.ptr, stream=_stream(), window=window)
    _sync()
    assert np.array_equal(dc.get(), st["n"]) and np.array_equal(dp.get(), st["period"]), (w, name)
    assert np.array_equal(_bits64(dd.get().reshape(n, 2)), _bits64(st["delta"])), (w, name)
    assert len(np.unique(st["period"])) >= 3


@pytest.mark.parametrize("w,name", DEEP_EDGE, ids=DEEP_EDGE_IDS)
def test_wide_deep_view_xbla_distance_normals_and_nucleus(gpu, w, name):
    """The extended-range kernels on the windows of test_wide_deep_view_counts, each against its own model through
    offsets(view, window): XBLA counts (deep_wide_bla_model), the distance estimate with the plain step and with XBLA
    (deep_wide_distance_model / _bla_model: assert_states_agree, as their GPU tests), normals with both (deep_wide_relief_model,
    bit for bit), periods and seeds (deep_wide_nucleus_model, bit for bit)."""
    import deep_wide_bla_model as X
    import deep_wide_distance_bla_model as XD
    import deep_wide_distance_model as WD
    import deep_wide_model as W
    import deep_wide_nucleus_model as WN
    import deep_wide_relief_model as WR
    mrd = 1000
    orbit, view, window = wide_case(w, name, mrd)
    shape = (window[3], window[2])
    n = shape[0] * shape[1]
    dr, di = W.offsets(view, window)
    tab = orbit.wide_table()
    xc = X.counts(*tab, dr, di, view.exp2, mrd, X.build(*tab, X.dcmax(view)))[0].reshape(shape)
    assert len(np.unique(xc)) >= 5
    dc = Guarded(np.int32, n)
    _sync()
    gpu.launch_deep_view(orbit, view, mrd, d_counts=dc.ptr, stream=_stream(), window=window, xbla=True)
    _sync()
    assert np.array_equal(dc.get(shape), xc), (w, name, "xbla counts")
    for model, launch, what in ((WD.model, gpu.launch_wide_view_distance, "distance"), (XD.model, gpu.launch_wide_view_distance_xbla, "distance xbla")):
        mrel, mn, st = model(orbit, view, mrd, window)
        drel, dc = Guarded(np.float64, n), Guarded(np.int32, n)
        _sync()
        launch(orbit, view, mrd, d_rel=drel.ptr, d_counts=dc.ptr, stream=_stream(), window=window)
        _sync()
        rel = drel.get(shape)
        assert np.array_equal(dc.get(shape), mn), (w, name, what)
        assert not np.isnan(rel).any() and (rel[mn == 0] == 0.0).all() and (rel >= 0.0).all(), (w, name, what)
        WD.assert_states_agree(rel, st, view.range_r, view.exp2, f"wide {what} {w} {name}")
    for xbla in (False, True):
        want, mn, _, _, _ = WR.model(orbit, view, mrd, window, xbla=xbla)
        dn, dc = Guarded(np.float64, 2 * n), Guarded(np.int32, n)
        _sync()
        gpu.launch_wide_view_normals(orbit, view, mrd, d_normals=dn.ptr, d_counts=dc.ptr, stream=_stream(), window=window, xbla=xbla)
        _sync()
        assert np.array_equal(dc.get(shape), mn), (w, name, xbla)
        got = dn.get(shape + (2,))
        assert np.array_equal(_bits64(got), _bits64(want)), (w, name, xbla, int((_bits64(got) != _bits64(want)).any(axis=2).sum()))
    st = WN.model(orbit, view, mrd, window)
    dp, dd, dc = Guarded(np.int32, n), Guarded(np.float64, 2 * n), Guarded(np.int32, n)
    _sync()
    gpu.launch_wide_view_nucleus(orbit, view, mrd, d_period=dp.ptr, d_delta=dd.ptr, d_counts=dc.ptr, stream=_stream(), window=window)
    _sync()
    assert np.array_equal(dc.get(), st["n"]) and np.array_equal(dp.get(), st["period"]), (w, name)
    assert np.array_equal(_bits64(dd.get().reshape(n, 2)), _bits64(st["delta"])), (w, name)


def _adaptive_deep_check(gpu, kind, s=2):
    """An adaptive render of a deep ("deep", BLA) or extended-range ("wide", XBLA) view of (2^32 - 1) // s samples per axis -- the
    finer view has 2^32 - 2, the most a render accepts -- at the far corner: adaptive_model.render_adaptive_window on the device's
    own smooth values of the halo and of the finer view's window, whose counts are held to the kind's model here."""
    import adaptive_model as A
    import deep_bla_model as BL
    import deep_model as D
    import deep_wide_bla_model as X
    import deep_wide_model as W
    from distributedmandelbrot_amd import DeepView, WideDeepView
    w = h = (2 ** 32 - 1) // s
    window = (w - 13, h - 11, 13, 11)
    if kind == "deep":
        mrd = 3000
        view = DeepView(DEEP_STEP * (w - 1), w, h, DEEP_STEP * (h - 1))
        dr, di = D.offsets(view, window)
        from fractions import Fraction
        from distributedmandelbrot_amd import DeepOrbit
        orbit = DeepOrbit(Fraction(ANCHOR[0]) - Fraction(float(dr[0])), Fraction(ANCHOR[1]) - Fraction(float(di[0])), mrd, min_span=DEEP_STEP / 4)
        fine, flag = DeepView(view.span_r, w * s, h * s, view.span_i), {"bla": True}
        zr, zi = orbit.table()

        def model(v, win):
            table = BL.build(zr, zi, BL.dcmax(v))
            return BL.counts(zr, zi, *D.offsets(v, win), mrd, table)[0].reshape(win[3], win[2])
    else:
        mrd = 1000
        orbit, view, _ = wide_case(w, None, mrd, h=h, window=window)
        fine, flag = WideDeepView(view.range_r, view.exp2, w * s, h * s, view.range_i), {"xbla": True}
        tab = orbit.wide_table()

        def model(v, win):
            return X.counts(*tab, *W.offsets(v, win), v.exp2, mrd, X.build(*tab, X.dcmax(v)))[0].reshape(win[3], win[2])
    assert fine.width == 2 ** 32 - 2
    hal = A.halo(window, w, h)
    samples = {}
    for key, v, win in (("halo", view, hal), ("fine", fine, tuple(s * x for x in window))):
        counts, _, nu, _ = gpu.compute_deep_view(orbit, v, mrd, window=win, want_bytes=False, want_smooth=True, **flag)
        assert np.array_equal(counts, model(v, win)), (kind, key)
        samples[key] = (counts, nu)
    assert len(np.unique(samples["fine"][0])) >= (20 if kind == "deep" else 5)
    launch = gpu.launch_render_deep_view_adaptive if kind == "deep" else gpu.launch_render_wide_view_adaptive
    for thr in (0, 24, 256):
        for rows in (0, 5):
            out, dm = Guarded(np.uint8, 4 * 13 * 11), Guarded(np.uint8, 13 * 11 + 1)
            _sync()
            launch(orbit, view, mrd, palette=SMOOTH_PAL, supersample=s, threshold=thr, d_rgba=out.ptr, d_mask=dm.ptr, stream=_stream(),
                   window=window, max_band_rows=rows, **flag)
            _sync()
            want, want_mask = A.render_adaptive_window(SMOOTH_PAL.entries, SMOOTH_PAL.inside, SMOOTH_PAL.scale, SMOOTH_PAL.offset, s, thr,
                                                       window, w, h, *samples["halo"], *samples["fine"])
            img, mask = out.get((11, 13, 4)), dm.get()[:143].reshape(11, 13)
            assert np.array_equal(mask, want_mask), (kind, thr, rows)
            assert np.array_equal(img, want), (kind, thr, rows, int((img != want).any(axis=2).sum()))


def test_deep_adaptive_render_at_the_largest_view(gpu):
    _adaptive_deep_check(gpu, "deep")


def test_wide_adaptive_render_at_the_largest_view(gpu):
    _adaptive_deep_check(gpu, "wide")
