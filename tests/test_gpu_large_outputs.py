"""Outputs that cross 2^32 bytes -- run with -m gpu.  The windows are the smallest whose int32 (float64, 16-byte) output holds byte
offsets on both sides of 2^32; the work stays small through mrd 16 to 64, not through fewer pixels.

Layout: an output is the upper part of one allocation that starts with a 2 GiB guard of 0xA5 and ends with a 64 MiB one.  A 32-bit
offset that wraps lands inside the output, one that is sign-extended at most 2 GiB below it: a wrong address is a failed
comparison here, never a stray store.  (A bytes output cannot reach 2^32 bytes -- a window has at most 2^31 pixels -- and sits
between 4 KiB guards.)  Both guards are compared on the device.

Reference, in two parts.  (i) The same window again as bands of at most 2^26 pixels through selector "asm" (families without
selectors: their one kernel), each into a small buffer, compared on the device with the matching slice: a window is bit-identical
to the whole view.  (ii) What anchors (i): the numpy reference of tests/geometry_model.py (the family's model for Julia and
deep views) on sampled rows -- the first, the last, the rows that hold byte offsets 2^32 - 1 and 2^32 with their neighbours, and for
the scan path the rows at which a wave's run of blocks starts anew because a 32-bit offset would pass 2^32 (run_cap in
csrc/mbk_scan.h) -- whole rows for plain views, the first and last 64 columns otherwise.

The statistics of the whole output (reduce_counts, counts_histogram over up to 2^31 counts) must equal the bands' sums.
A test holds about 7.5 GiB of device memory and skips only where less than 12 GiB are free."""
import numpy as np
import pytest

import deep_model as D
import distance_model as DM
import geometry_model as G
import julia_model as J
import relief_model as RM
import smooth_truth as T
from distributedmandelbrot_amd import DeepOrbit, DeepView, View

pytestmark = pytest.mark.gpu

FRONT, BACK, SMALL = 2 ** 31, 2 ** 26, 4096
BAND_PIXELS = 2 ** 26
FULL = (-2.0, -1.5, 3.0, 3.0)
BELOW = (-2.0, -2.0, 4.0, 0.9)         # all exterior (no probe pixel outlives the light pass), counts from 1 to 8 and more
JULIA_C = (-0.8, 0.156)
PATTERN = -0x5A5A5A5A5A5A5A5B           # 0xA5 eight times, as int64


def _torch():
    import torch
    return torch


@pytest.fixture(autouse=True)
def enough_memory():
    torch = _torch()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, 12 needed")
    yield
    # what the device holds now: torch's cache still has the test's buffers, the library its scratch
    free_now, total = torch.cuda.mem_get_info()
    USED["peak_in_use"] = max(USED["peak_in_use"], total - free_now)
    USED["peak_torch"] = max(USED["peak_torch"], torch.cuda.max_memory_allocated())
    torch.cuda.empty_cache()


USED = {"peak_in_use": 0, "peak_torch": 0}


@pytest.fixture(scope="module", autouse=True)
def report_memory():
    yield
    print(f"\npeak device memory in use at the end of a test {USED['peak_in_use'] / 2 ** 30:.2f} GiB, "
          f"peak torch allocation {USED['peak_torch'] / 2 ** 30:.2f} GiB")


class Big:
    """n elements of itemsize bytes behind a guard of `front` bytes and before one of `back` bytes, all 0xA5 to begin with."""

    def __init__(self, itemsize, n, front=FRONT, back=BACK):
        torch = _torch()
        self.nbytes, self.front = int(n) * itemsize, front
        assert self.nbytes % 8 == 0
        self.t = torch.full((front + self.nbytes + back,), 0xA5, dtype=torch.uint8, device="cuda:0")

    @property
    def ptr(self):
        return self.t.data_ptr() + self.front

    def body(self, dtype):
        return self.t[self.front:self.front + self.nbytes].view(dtype)

    def guards_intact(self):
        lo, hi = self.t[:self.front].view(_torch().int64), self.t[self.front + self.nbytes:].view(_torch().int64)
        return not bool(lo.ne(PATTERN).any()) and not bool(hi.ne(PATTERN).any())


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _sync():
    _torch().cuda.synchronize()


def sample_rows(ncols, nrows, itemsize, extra=()):
    """The first and last rows, the rows holding byte offsets 2^32 - 1 and 2^32 and their neighbours, two rows from the middle of
    the window (in these shapes all the others lie at the view's ends), and `extra`."""
    lo, hi = (2 ** 32 - 1) // (ncols * itemsize), 2 ** 32 // (ncols * itemsize)
    assert 0 < lo <= hi < nrows - 1, "the output does not cross 2^32 bytes"
    rows = {0, 1, nrows - 2, nrows - 1, lo - 1, lo, hi, hi + 1, nrows // 2, nrows // 3} | {r for r in extra if 0 <= r < nrows}
    return sorted(rows)


def bands(ncols, nrows):
    per = BAND_PIXELS // ncols
    return [(r0, min(per, nrows - r0)) for r0 in range(0, nrows, per)]


def check_statistics(gpu, counts, pieces, mrd):
    """reduce_counts and counts_histogram of the whole int32 output against the sums over `pieces` (slices of it, as the bands
    were compared equal to them)."""
    torch = _torch()
    n = counts.numel()
    assert n <= 2 ** 31
    st = gpu.reduce_counts(counts.data_ptr(), n, mrd, stream=_stream())
    its = nev = 0
    hist = torch.zeros(mrd, dtype=torch.int64, device="cuda:0")
    parts = torch.zeros(mrd, dtype=torch.int64, device="cuda:0")
    for piece in pieces:
        s = gpu.reduce_counts(piece.data_ptr(), piece.numel(), mrd, stream=_stream())
        its, nev = its + s.pixel_iterations, nev + s.never_pixels
        gpu.counts_histogram(piece.data_ptr(), piece.numel(), mrd, parts.data_ptr(), stream=_stream())
    gpu.counts_histogram(counts.data_ptr(), n, mrd, hist.data_ptr(), stream=_stream())
    _sync()
    assert (st.pixel_iterations, st.never_pixels) == (its, nev)
    assert torch.equal(hist, parts) and int(hist.sum()) == n and int(hist[0]) == nev
    return its, nev


def rle_runs_of_bands(byts, pieces):
    """The runs of equal bytes of the whole output, row-major, summed over the bands on the device: a band's own runs, less one
    for every band whose first byte continues the run that ends the band before it."""
    total, last = 0, None
    for r0, nr in pieces:
        flat = byts[r0:r0 + nr].reshape(-1)
        total += 1 + int((flat[1:] != flat[:-1]).sum())
        if last is not None and int(flat[0]) == last:
            total -= 1
        last = int(flat[-1])
    return total


# ---- plain views: counts and bytes through every route ----------------------------------------------------------------------------

def scan_restart_rows(gpu, ncols, nrows, strip, with_counts):
    """Rows at which a wave of tile_light_kernel starts a new run because the next 32-bit offset would pass 2^32, from the formulas
    of csrc/mbk_scan.h and launch_scan_t, for every resident grid the launch may have had (the occupancy of the finish-in-place form
    is not reported: 4 to 32 workgroups per CU, and what scan_occupancy does report)."""
    cus = gpu.info()["compute_units"]
    rows = set()
    for per_cu in set(range(4, 33, 4)) | set(gpu.scan_occupancy().values()):
        bw, bh = (64, 1) if strip else (8, 8)
        regions_x, regions_y = (ncols + bw - 1) // bw, (nrows + bh - 1) // bh
        stride_by = min(cus * per_cu // regions_x, regions_y)
        if stride_by == 0:
            continue
        oscale = 4 if with_counts else 1
        einc = stride_by * bh * ncols * oscale
        assert einc < 2 ** 31
        run_cap = (0xffffffff - ((bh - 1) * ncols + bw - 1) * oscale) // einc
        for m in range(1, 4):
            r = m * run_cap * stride_by * bh
            rows |= {r - 1, r, r + bh, r + stride_by * bh - 1, r + stride_by * bh}
    return {r for r in rows if 0 <= r < nrows}


def run_plain(gpu, area, ncols, nrows, mrd, kernel, options, with_bytes, extra_rows=()):
    torch = _torch()
    view, n = View(*area, ncols, nrows), ncols * nrows
    saved = {k: gpu.get_option(k) for k in options}
    dc = Big(4, n)
    db = Big(1, n, SMALL, SMALL) if with_bytes else None
    try:
        for k, v in options.items():
            gpu.set_option(k, v)
        _sync()
        gpu.launch_view(view, mrd, d_counts=dc.ptr, d_bytes=db.ptr if with_bytes else 0, stream=_stream(), kernel=kernel)
        _sync()
    finally:
        for k, v in saved.items():
            gpu.set_option(k, v)
    assert dc.guards_intact() and (db is None or db.guards_intact()), "a guard was written"
    counts = dc.body(torch.int32).view(nrows, ncols)
    byts = db.body(torch.uint8).view(nrows, ncols) if with_bytes else None
    # (i) bands through "asm"
    bc, bb = Big(4, BAND_PIXELS, SMALL, SMALL), Big(1, BAND_PIXELS, SMALL, SMALL)
    for r0, nr in bands(ncols, nrows):
        gpu.launch_view(view, mrd, d_counts=bc.ptr, d_bytes=bb.ptr if with_bytes else 0, stream=_stream(), window=(0, r0, ncols, nr), kernel="asm")
        _sync()
        assert torch.equal(bc.body(torch.int32)[:nr * ncols].view(nr, ncols), counts[r0:r0 + nr]), (kernel, options, r0)
        if with_bytes:
            assert torch.equal(bb.body(torch.uint8)[:nr * ncols].view(nr, ncols), byts[r0:r0 + nr]), (kernel, options, r0)
    assert bc.guards_intact() and bb.guards_intact()
    # (ii) the numpy reference on whole sampled rows
    rows = sample_rows(ncols, nrows, 4, extra_rows)
    idx = torch.tensor(rows, device="cuda:0")
    got_c = counts[idx].cpu().numpy()
    got_b = byts[idx].cpu().numpy() if with_bytes else None
    xr = G.axis_sample(area[0], area[2], ncols, np.arange(ncols, dtype=np.uint64))
    xi = G.axis_sample(area[1], area[3], nrows, np.array(rows, dtype=np.uint64))
    from oracle.oracle import numpy_escape, numpy_quantise
    want = numpy_escape(xr[None, :], xi[:, None], mrd).reshape(len(rows), ncols)
    assert np.array_equal(got_c, want), (kernel, options, [rows[i] for i in np.flatnonzero((got_c != want).any(axis=1))])
    if with_bytes:
        assert np.array_equal(got_b, numpy_quantise(want, mrd)), (kernel, options)
    its, nev = check_statistics(gpu, counts, [counts[r0:r0 + nr] for r0, nr in bands(ncols, nrows)], mrd)
    if with_bytes:
        # the launch's own statistics, rle_runs among them, against the bands' sums.  A launch form returns none, so the same
        # window goes once more through the synchronous form, bytes only (the kernel then adds up the statistics itself and writes
        # no counts), on a context of its own and after this test's buffers are gone: its slot buffers take their place.
        from distributedmandelbrot_amd import MandelbrotDevice
        runs = rle_runs_of_bands(byts, bands(ncols, nrows))
        del counts, byts, dc, db, bc, bb, idx
        torch.cuda.empty_cache()
        with MandelbrotDevice(0) as dev:
            for k, v in options.items():
                dev.set_option(k, v)
            _, hb, st = dev.compute_view(view, mrd, want_counts=False, kernel=kernel)
        assert (st.rle_runs, st.pixel_iterations, st.never_pixels) == (runs, its, nev), (kernel, options)
        assert np.array_equal(hb[rows], numpy_quantise(want, mrd)), (kernel, options)
    return want


SCAN_SHAPE = (512, 2 ** 21 + 64)


@pytest.mark.parametrize("with_bytes", [False, True], ids=["counts", "counts+bytes"])
@pytest.mark.parametrize("waves", [8, 1], ids=["scan_waves8", "scan_waves1"])
def test_scan_finish_in_place_row_strips(gpu, with_bytes, waves):
    """All exterior, 512 columns: 64 x 1 strips, one launch.  A wave's run of strips would span more than 2^32 bytes of the int32
    output: run_cap ends it before the offset wraps (scan_waves 1: a grid of 4 workgroups per CU, so that the rows at which that
    happens are known; 8, the default: every grid the occupancy may have given)."""
    ncols, nrows = SCAN_SHAPE
    extra = scan_restart_rows(gpu, ncols, nrows, True, True)
    assert any(r > nrows - 4096 for r in extra)          # a run does start anew inside the window
    want = run_plain(gpu, BELOW, ncols, nrows, 32, "scan", {"scan_inline": 1, "scan_strip": 1, "scan_waves": waves}, with_bytes, extra)
    assert len(np.unique(want)) >= 6 and not (want == 0).any()


@pytest.mark.parametrize("area,options", [(BELOW, {"scan_inline": 1, "scan_strip": 0}), (FULL, {})], ids=["blocks_in_place", "two_pass"])
def test_scan_8x8_regions(gpu, area, options):
    ncols, nrows = SCAN_SHAPE
    extra = scan_restart_rows(gpu, ncols, nrows, False, True)
    want = run_plain(gpu, area, ncols, nrows, 32, "scan", dict(options, scan_waves=1), True, extra)
    assert len(np.unique(want)) >= 6 and (area == BELOW or (want == 0).any())


WIDE_SHAPE = (16384, 65544)


@pytest.mark.parametrize("with_bytes", [False, True], ids=["counts", "counts+bytes"])
def test_units_kernel(gpu, with_bytes):
    ncols, nrows = WIDE_SHAPE
    assert ncols // 8 == 2048 and (nrows + 7) // 8 <= 0xffff and 32 > 2 * 8          # (mrd above twice the probe depth: the units gate)
    want = run_plain(gpu, FULL, ncols, nrows, 32, "group", {"order": 3, "units_min_light": 0, "probe_steps": 8}, with_bytes)
    assert (want == 0).any() and len(np.unique(want)) >= 20


@pytest.mark.parametrize("kernel,options", [("group", {"order": 3, "units_min_light": 65536, "probe_steps": 8}), ("group", {"order": 0}), ("asm", {}), ("simple", {}),
                                            ("refill", {})], ids=["group_classify_list", "group_image_order", "asm", "simple", "refill"])
def test_block_kernels(gpu, kernel, options):
    ncols, nrows = WIDE_SHAPE
    want = run_plain(gpu, FULL, ncols, nrows, 32, kernel, options, False)
    assert (want == 0).any() and len(np.unique(want)) >= 20


# ---- the other families ---------------------------------------------------------------------------------------------------------------

def edge_columns(ncols):
    return np.concatenate([np.arange(64), np.arange(ncols - 64, ncols)])


def test_plain_smooth():
    """float64: 16 384 x 32 776 values cross 2^32 bytes."""
    torch = _torch()
    from distributedmandelbrot_amd import MandelbrotDevice
    ncols, nrows, mrd = 16384, 32776, 32
    view = View(*FULL, ncols, nrows)
    with MandelbrotDevice(0) as gpu:
        out = Big(8, ncols * nrows)
        _sync()
        gpu.launch_view_smooth(view, mrd, d_smooth=out.ptr, stream=_stream())
        _sync()
        assert out.guards_intact()
        nu = out.body(torch.float64).view(nrows, ncols)
        band = Big(8, BAND_PIXELS, SMALL, SMALL)
        for r0, nr in bands(ncols, nrows):
            gpu.launch_view_smooth(view, mrd, d_smooth=band.ptr, stream=_stream(), window=(0, r0, ncols, nr), kernel="asm")
            _sync()
            assert torch.equal(band.body(torch.int64)[:nr * ncols].view(nr, ncols), nu[r0:r0 + nr].view(torch.int64)), r0
        assert band.guards_intact()
        rows = sample_rows(ncols, nrows, 8)
        got = nu[torch.tensor(rows, device="cuda:0")].cpu().numpy()
    # whole rows against the libm value of the formula on the reference's counts and |z|^2 (assert_pair: zeros where the count
    # is 0, both sides' bounds), the first and last 64 columns against the correctly rounded value (assert_within)
    cols = edge_columns(ncols)
    for k, r in enumerate(rows):
        oc, mag = G.window_escape((*FULL, ncols, nrows), (0, r, ncols, 1), mrd)
        T.assert_pair(got[k:k + 1], D.smooth_from(oc, mag), oc, f"smooth row {r}")
        T.assert_within(got[k, cols], oc[0, cols], mag[0, cols], f"smooth row {r}, edge columns")


def test_plain_normals():
    """16 bytes per pixel: 8 192 x 32 776."""
    torch = _torch()
    from distributedmandelbrot_amd import MandelbrotDevice
    ncols, nrows, mrd = 8192, 32776, 32
    area = FULL
    view = View(*area, ncols, nrows)
    with MandelbrotDevice(0) as gpu:
        out = Big(16, ncols * nrows)
        _sync()
        gpu.launch_view_normals(view, mrd, d_normals=out.ptr, stream=_stream())
        _sync()
        assert out.guards_intact()
        nrm = out.body(torch.int64).view(nrows, 2 * ncols)
        band = Big(16, BAND_PIXELS, SMALL, SMALL)
        for r0, nr in bands(ncols, nrows):
            gpu.launch_view_normals(view, mrd, d_normals=band.ptr, stream=_stream(), window=(0, r0, ncols, nr))
            _sync()
            assert torch.equal(band.body(torch.int64)[:2 * nr * ncols].view(nr, 2 * ncols), nrm[r0:r0 + nr]), r0
        assert band.guards_intact()
        rows = sample_rows(ncols, nrows, 16)
        got = nrm[torch.tensor(rows, device="cuda:0")].cpu().numpy().view(np.float64).reshape(len(rows), ncols, 2)
    cols = edge_columns(ncols)
    xr = G.axis_sample(area[0], area[2], ncols, cols.astype(np.uint64))
    xi = G.axis_sample(area[1], area[3], nrows, np.array(rows, dtype=np.uint64))
    st = DM.states(np.tile(xr, xi.size), np.repeat(xi, xr.size), mrd)
    want = RM.normal(st["zr"], st["zi"], st["dr"], st["di"], st["n"]).reshape(len(rows), cols.size, 2)
    # bit for bit, as tests/test_gpu_relief.py holds the normals to this model
    assert np.array_equal(got[:, cols].view(np.uint64), want.view(np.uint64))
    assert (st["n"] > 0).any()


def test_julia_counts(gpu):
    torch = _torch()
    ncols, nrows = WIDE_SHAPE
    mrd, area = 32, (-1.6, -1.2, 3.2, 2.4)
    view = View(*area, ncols, nrows)
    out = Big(4, ncols * nrows)
    _sync()
    gpu.launch_julia_view(view, JULIA_C, mrd, d_counts=out.ptr, stream=_stream())
    _sync()
    assert out.guards_intact()
    counts = out.body(torch.int32).view(nrows, ncols)
    band = Big(4, BAND_PIXELS, SMALL, SMALL)
    for r0, nr in bands(ncols, nrows):
        gpu.launch_julia_view(view, JULIA_C, mrd, d_counts=band.ptr, stream=_stream(), window=(0, r0, ncols, nr), kernel="asm")
        _sync()
        assert torch.equal(band.body(torch.int32)[:nr * ncols].view(nr, ncols), counts[r0:r0 + nr]), r0
    assert band.guards_intact()
    rows = sample_rows(ncols, nrows, 4)
    got = counts[torch.tensor(rows, device="cuda:0")].cpu().numpy()
    xr = G.axis_sample(area[0], area[2], ncols, np.arange(ncols, dtype=np.uint64))
    xi = G.axis_sample(area[1], area[3], nrows, np.array(rows, dtype=np.uint64))
    want, _ = J.julia_counts(xr[None, :], xi[:, None], JULIA_C[0], JULIA_C[1], mrd)
    assert np.array_equal(got, want) and len(np.unique(want)) >= 20
    check_statistics(gpu, counts, [counts[r0:r0 + nr] for r0, nr in bands(ncols, nrows)], mrd)


def test_deep_view_plain_step(gpu):
    torch = _torch()
    ncols, nrows = WIDE_SHAPE
    mrd = 16
    orbit = DeepOrbit("-0.5", "0", mrd, min_span=1e-6)
    view = DeepView(3.0, ncols, nrows, 3.0)
    out = Big(4, ncols * nrows)
    _sync()
    gpu.launch_deep_view(orbit, view, mrd, d_counts=out.ptr, stream=_stream())
    _sync()
    assert out.guards_intact()
    counts = out.body(torch.int32).view(nrows, ncols)
    band = Big(4, BAND_PIXELS, SMALL, SMALL)
    for r0, nr in bands(ncols, nrows):
        gpu.launch_deep_view(orbit, view, mrd, d_counts=band.ptr, stream=_stream(), window=(0, r0, ncols, nr))
        _sync()
        assert torch.equal(band.body(torch.int32)[:nr * ncols].view(nr, ncols), counts[r0:r0 + nr]), r0
    assert band.guards_intact()
    rows = sample_rows(ncols, nrows, 4)
    cols = edge_columns(ncols)
    got = counts[torch.tensor(rows, device="cuda:0")].cpu().numpy()[:, cols]
    zr, zi = orbit.table()
    dr = D.axis_offsets(ncols, view.span_r, cols)
    di = D.axis_offsets(nrows, view.span_i, np.array(rows))
    want, _ = D.model_counts(zr, zi, np.tile(dr, len(rows)), np.repeat(di, cols.size), mrd)
    assert np.array_equal(got.ravel(), want) and len(np.unique(want)) >= 3
    check_statistics(gpu, counts, [counts[r0:r0 + nr] for r0, nr in bands(ncols, nrows)], mrd)
