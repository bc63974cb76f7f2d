"""CPU tests of density views (include/mbk.h, "Density views"): the host twins -- compiled from the functions the kernels
use -- against the numpy restatement of the contract in tests/density_model.py, exactly."""
import ctypes as C

import numpy as np
import pytest

import density_model as M

from distributedmandelbrot_amd import DensityTarget, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import density_cell_host, density_host
from distributedmandelbrot_amd.image import resolve_density_host

VIEW = View(-2.0, -1.25, 3.0, 2.5, 96, 64)
MRD = 200
WIDE = DensityTarget(-2.0, -1.5, 3.0, 3.0, 48, 40)
NARROW = DensityTarget(-0.5, 0.5, 0.5, 0.5, 48, 40)     # [-0.5, 0] x [0.5, 1]: most points miss it
DISC = DensityTarget(-2.5, -2.5, 5.0, 5.0, 40, 40)      # contains the disc of radius 2
POW2 = DensityTarget(-2.0, -2.0, 4.0, 4.0, 8, 16)       # inv_r = 2, inv_i = 4: every product exact


@pytest.fixture(scope="module")
def view_counts(oracle):
    """The counts of VIEW, once: from the model, and held to the C oracle so that the model's samples are the library's."""
    xs, ys = M.axes(VIEW)
    cr, ci = np.meshgrid(xs, ys)
    n = M.counts(cr, ci, MRD)
    oc = oracle.view(VIEW.start_r, VIEW.start_i, VIEW.range_r, VIEW.range_i, VIEW.width, VIEW.height, MRD)[0]
    assert np.array_equal(n, oc.reshape(n.shape))
    return n


def _ulp_neighbours(x):
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


@pytest.mark.parametrize("target", [WIDE, NARROW, POW2, DensityTarget(-2.0, -1.5, 3.0, 3.0, 7, 3), DensityTarget(0.1, -0.3, 0.7, 1.9, 1, 5),
                                    DensityTarget(-1e-3, 1e-3, 3e-3, 1e-3, 1, 1)])
def test_cell_rule(target):
    """Points on `start`, on the right and the top edge and one ulp either side of each, negative tx, huge |c|, infinities and
    NaN handed in directly, with W != H and W = 1."""
    right, top = target.start_r + target.range_r, target.start_i + target.range_i
    xs = (_ulp_neighbours(target.start_r) + _ulp_neighbours(right) + [target.start_r + 0.37 * target.range_r, target.start_r - 1.0,
          -0.0, 0.0, 1e77, -1e77, 1.7e308, np.inf, -np.inf, np.nan])
    ys = (_ulp_neighbours(target.start_i) + _ulp_neighbours(top) + [target.start_i + 0.61 * target.range_i, target.start_i - 1.0,
          -0.0, 0.0, 1e77, -1e77, np.inf, -np.inf, np.nan])
    zr, zi = [a.ravel() for a in np.meshgrid(np.array(xs), np.array(ys))]
    inside, cx, cy = M.cells(target, zr, zi)
    assert inside.any() and not inside.all()
    for k in range(zr.size):
        got = density_cell_host(target, (zr[k], zi[k]))
        want = (int(cx[k]), int(cy[k])) if inside[k] else None
        assert got == want, (zr[k], zi[k], got, want)
    # the corner cell and the edges, spelled out where inv_* and the edges are exact (elsewhere the formula decides: the model)
    assert density_cell_host(target, (target.start_r, target.start_i)) == (0, 0)
    assert density_cell_host(target, (float(np.nextafter(target.start_r, -np.inf)), target.start_i)) is None
    if target in (NARROW, POW2):
        assert density_cell_host(target, (right, target.start_i)) is None
        assert density_cell_host(target, (target.start_r, top)) is None


@pytest.mark.parametrize("target", [WIDE, NARROW], ids=["wide", "narrow"])
def test_accumulate_host_equals_the_model(target, view_counts):
    want, dep, drop, n = M.accumulate(VIEW, target, MRD, n=view_counts)
    got, ds = density_host(VIEW, target, MRD)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert (ds.deposits, ds.dropped) == (dep, drop)
    assert dep + drop == int(n[n > 0].sum()) and dep == int(want.sum()) and drop > 0
    if target is NARROW:
        assert drop > 5 * dep   # most points miss it
    # a window and the rest of the view add up to the view; the host twin ADDS
    part, _ = density_host(VIEW, target, MRD, window=(0, 0, VIEW.width, 29))
    rest, _ = density_host(VIEW, target, MRD, window=(0, 29, VIEW.width, VIEW.height - 29), out=part)
    assert rest is part or np.shares_memory(rest, part)
    assert np.array_equal(rest, want)


def test_a_target_that_holds_the_disc_drops_nothing(view_counts, oracle):
    inner = View(-1.9, -1.2, 2.4, 2.4, 48, 40)   # inside the target, and |c| <= 2.25 < 2.5
    want, dep, drop, n = M.accumulate(inner, DISC, MRD)
    got, ds = density_host(inner, DISC, MRD)
    assert np.array_equal(got, want)
    assert ds.dropped == 0 == drop
    # ... and the table's sum is the sum of n, which is pixel_iterations - (mrd - 1) never_pixels of mbk_stats
    total = oracle.view(inner.start_r, inner.start_i, inner.range_r, inner.range_i, inner.width, inner.height, MRD)[2]
    never = int((n == 0).sum())
    assert int(got.sum()) == ds.deposits == int(n.sum()) == total - (MRD - 1) * never


@pytest.mark.parametrize("band", [(1, 0), (1, 1), (5, 5), (MRD - 1, MRD - 1), (10, 50)])
def test_filters(band, view_counts):
    lo, hi = band
    want, dep, drop, n = M.accumulate(VIEW, WIDE, MRD, lo, hi, n=view_counts)
    got, ds = density_host(VIEW, WIDE, MRD, min_count=lo, max_count=hi)
    assert np.array_equal(got, want) and (ds.deposits, ds.dropped) == (dep, drop)
    q = M.qualify(n, MRD, lo, hi)
    assert dep + drop == int(n[q].sum())
    if band != (MRD - 1, MRD - 1):
        assert dep > 0


def test_disjoint_count_bands_add_up_to_their_union():
    whole, ws = density_host(VIEW, WIDE, MRD)
    acc = np.zeros_like(whole)
    deposits = 0
    for lo, hi in [(1, 1), (2, 4), (5, 5), (6, 9), (10, 50), (51, MRD - 2), (MRD - 1, MRD - 1)]:
        _, ds = density_host(VIEW, WIDE, MRD, min_count=lo, max_count=hi, out=acc)
        deposits += ds.deposits
    assert np.array_equal(acc, whole) and deposits == ws.deposits


@pytest.mark.parametrize("mrd", [0, 1])
def test_mrd_0_and_1_deposit_nothing(mrd):
    got, ds = density_host(VIEW, WIDE, mrd)
    assert not got.any() and (ds.deposits, ds.dropped) == (0, 0)


def _palette(n, seed=5):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (n, 4)).astype(np.uint8)


@pytest.mark.parametrize("mode", ["linear", "sqrt"])
@pytest.mark.parametrize("factor", [1, 2, 4, 8])
def test_resolve_twin_equals_the_model(mode, factor):
    """Both g, every factor; t below 0, at and above n - 1; a table that holds 0 and 2^32 - 1."""
    rs = np.random.RandomState(11 + factor)
    table = rs.randint(0, 900, (16, 24)).astype(np.uint32)
    table[0, :6] = [0, 1, 2 ** 32 - 1, 2 ** 31, 4, 9]
    table[5, 3] = 2 ** 32 - 1
    entries = _palette(37)
    g = (lambda v: np.sqrt(np.float64(v))) if mode == "sqrt" else np.float64
    for scale, offset in [(36.0 / float(g(899)), 0.0),     # the random cells span the palette
                          (0.125, -3.0),                    # t < 0 for small cells
                          (36.0 / float(g(4)), 0.0),        # v = 4 lands on n - 1 exactly
                          (2.0 ** 80, 2.0 ** 20), (2.0 ** -30, 0.25)]:
        pal = Palette(entries, scale=scale, offset=offset)
        want = M.render(entries, scale, offset, mode, factor, table)
        got = resolve_density_host(pal, table, mode=mode, factor=factor)
        assert got.shape == want.shape and np.array_equal(got, want), (scale, offset)
    # Palette.for_density: the largest cell reaches the last entry, the empty cell the first
    small = table.copy()
    small[small >= 2 ** 31] = 0
    pal = Palette(entries).for_density(int(small.max()), mode)
    img = resolve_density_host(pal, small, mode=mode, factor=1)
    assert np.array_equal(img[small == small.max()][0], entries[-1]) and np.array_equal(img[small == 0][0], entries[0])
    assert np.array_equal(img, M.render(entries, pal.scale, pal.offset, mode, 1, small))


def _accumulate_status(view, target, mrd, lo, hi, table=True):
    lib = L.load()
    cv = None if view is None else C.byref(L.mbk_view(*view))
    ct = None if target is None else C.byref(L.mbk_density_target(*target))
    n = 1 if target is None else max(target[4] * target[5], 1)
    buf = np.full(min(n, 1 << 16), 7, np.uint32)
    st = lib.mbk_density_accumulate_host(cv, ct, mrd, lo, hi, buf.ctypes.data if table else None, None)
    assert (buf == 7).all() or st == L.MBK_OK   # a refusal writes nothing
    return st


V = (-2.0, -1.25, 3.0, 2.5, 12, 8, 0, 0, 12, 8)
T = (-2.0, -1.5, 3.0, 3.0, 6, 5)


def test_refusals_of_the_host_twins():
    ok, bad = L.MBK_OK, L.MBK_ERR_INVALID
    assert _accumulate_status(V, T, 50, 1, 0) == ok
    assert _accumulate_status(V, T, 50, 1, 49) == ok and _accumulate_status(V, T, 50, 49, 49) == ok
    assert _accumulate_status(V, T, 0, 1, 0) == ok and _accumulate_status(V, T, 1, 1, 0) == ok
    # NULL pointers
    assert _accumulate_status(None, T, 50, 1, 0) == bad
    assert _accumulate_status(V, None, 50, 1, 0) == bad
    assert _accumulate_status(V, T, 50, 1, 0, table=False) == bad
    # the count interval
    assert _accumulate_status(V, T, 50, 0, 0) == bad                # min_count == 0
    assert _accumulate_status(V, T, 50, 6, 5) == bad                # min_count > max_count
    assert _accumulate_status(V, T, 50, 50, 0) == bad               # ... after the substitution (mrd - 1 = 49)
    assert _accumulate_status(V, T, 50, 1, 50) == bad               # max_count >= mrd
    assert _accumulate_status(V, T, 2, 1, 2) == bad
    assert _accumulate_status(V, T, 1, 3, 2) == bad
    assert _accumulate_status(V, T, 2 ** 31, 1, 0) == bad           # mrd >= 2^31
    # the target's geometry
    for t in [(-2.0, -1.5, 3.0, 3.0, 0, 5), (-2.0, -1.5, 3.0, 3.0, 6, 0), (-2.0, -1.5, 0.0, 3.0, 6, 5), (-2.0, -1.5, 3.0, -3.0, 6, 5),
              (-2.0, -1.5, np.inf, 3.0, 6, 5), (-2.0, -1.5, 3.0, np.nan, 6, 5), (np.nan, -1.5, 3.0, 3.0, 6, 5),
              (-2.0, np.inf, 3.0, 3.0, 6, 5), (-2.0, -1.5, 3.0, 3.0, 1 << 14, (1 << 14) + 1)]:
        assert _accumulate_status(V, t, 50, 1, 0) == bad, t
    assert _accumulate_status(V, (-2.0, -1.5, 3.0, 3.0, 1 << 8, 1 << 8), 3, 1, 0) == ok
    # whatever mbk_view_launch refuses in a view
    for v in [(-2.0, -1.25, 3.0, 2.5, 0, 8, 0, 0, 0, 8), (-2.0, -1.25, 3.0, 2.5, 12, 8, 0, 0, 0, 8), (-2.0, -1.25, 3.0, 2.5, 12, 8, 4, 0, 12, 8),
              (np.nan, -1.25, 3.0, 2.5, 12, 8, 0, 0, 12, 8), (-2.0, -1.25, 1e300, 2.5, 12, 8, 0, 0, 12, 8)]:
        assert _accumulate_status(v, T, 50, 1, 0) == bad, v
    # the cell twin: NULL outputs, a bad target
    lib = L.load()
    cx, cy, ins = C.c_uint32(9), C.c_uint32(9), C.c_int(9)
    good = L.mbk_density_target(*T)
    assert lib.mbk_density_cell_host(C.byref(good), 0.0, 0.0, C.byref(cx), C.byref(cy), C.byref(ins)) == ok and ins.value == 1
    assert lib.mbk_density_cell_host(None, 0.0, 0.0, C.byref(cx), C.byref(cy), C.byref(ins)) == bad
    assert lib.mbk_density_cell_host(C.byref(good), 0.0, 0.0, None, C.byref(cy), C.byref(ins)) == bad
    assert lib.mbk_density_cell_host(C.byref(good), 0.0, 0.0, C.byref(cx), C.byref(cy), None) == bad
    with pytest.raises(MbkError):
        density_cell_host(DensityTarget(0.0, 0.0, -1.0, 1.0, 4, 4), (0.0, 0.0))


def test_refusals_of_the_resolve_twin():
    entries = _palette(16)
    table = np.arange(64, dtype=np.uint32).reshape(8, 8)
    assert resolve_density_host(Palette(entries), table).shape == (8, 8, 4)
    lib = L.load()
    out = np.full((8, 8, 4), 7, np.uint8)

    def status(mode=1, factor=1, pal=entries, n=16, scale=1.0, offset=0.0, w=8, h=8, tab=table, dst=out):
        spec = L.mbk_density_render_spec(mode, factor, None if pal is None else pal.ctypes.data, n, scale, offset)
        st = lib.mbk_density_resolve_host(C.byref(spec), w, h, None if tab is None else tab.ctypes.data,
                                          None if dst is None else dst.ctypes.data)
        return st

    bad = L.MBK_ERR_INVALID
    assert status() == L.MBK_OK
    out[:] = 7
    for kw in [dict(mode=2), dict(factor=3), dict(factor=0), dict(factor=16), dict(pal=None), dict(n=1), dict(n=65537), dict(scale=0.0),
               dict(scale=-1.0), dict(scale=2.0 ** 81), dict(scale=np.nan), dict(offset=2.0 ** 21), dict(offset=np.nan), dict(w=0),
               dict(h=0), dict(w=1 << 15, h=1 << 14), dict(factor=8, w=8, h=4), dict(factor=4, w=6, h=8), dict(tab=None), dict(dst=None)]:
        assert status(**kw) == bad, kw
    assert lib.mbk_density_resolve_host(None, 8, 8, table.ctypes.data, out.ctypes.data) == bad
    assert (out == 7).all()


# ---- the case table of the GPU tests (tests/density_cases.py), checked where no GPU is needed --------------------------------

def test_the_gpu_case_table_reaches_what_it_claims():
    import density_cases as DC
    names = {c.name for c in DC.CASES}
    empty = {"mrd0", "mrd1", "interior", "mrd258_top", "n255_256", "n256_257", "n128"}   # ENDS has no sample with n >= 63
    assert empty <= names
    for case in DC.CASES:
        want, dep, drop, nq = DC.expected(case)
        assert (dep > 0) == (case.name not in empty), case.name
        assert dep + drop == int(nq.sum())
        if not case.init:
            assert int(want.sum()) == dep
    bands = lambda name: sorted({int(v).bit_length() - 1 for v in DC.expected(DC.BY_NAME[name])[3]})
    for name in ("wide", "narrow", "big_rows", "t175"):
        assert bands(name) == list(range(8)) and len(np.unique(DC.expected(DC.BY_NAME[name])[3])) >= 8
    assert DC.expected(DC.BY_NAME["wide"])[3].size > 256                    # more than one workgroup of the list passes
    assert DC.SMALL.width * DC.SMALL.height == 117 and 0 < DC.expected(DC.BY_NAME["partial"])[3].size % 64
    assert bands("mrd2") == [0] and bands("mrd3") == [0, 1] and bands("mrd3_top") == [1]
    assert bands("n7_8") == [2, 3] and bands("n15_16") == [3, 4] and bands("n31_32") == [4, 5]   # 2^k - 1 against 2^k
    assert bands("n8_9") == [3] and bands("n16") == [4] and bands("n128_view") == [7]
    assert 0 < DC.expected(DC.BY_NAME["sparse"])[3].size < 64
    far = DC.expected(DC.BY_NAME["far"])
    assert (far[3] == 1).all() and far[3].size == 256 and far[2] == 0      # the list equals the window
    assert np.array_equal(DC.expected(DC.BY_NAME["big_rows"])[0], DC.expected(DC.BY_NAME["big_whole"])[0])
    assert np.array_equal(DC.expected(DC.BY_NAME["big_cols"])[0], DC.expected(DC.BY_NAME["big_whole"])[0])
    assert np.array_equal(DC.expected(DC.BY_NAME["big_twice"])[0], 2 * DC.expected(DC.BY_NAME["big_once"])[0])
    assert DC.expected(DC.BY_NAME["one_cell"])[2] == 0 == DC.expected(DC.BY_NAME["four_cells"])[2]
    t175 = DC.expected(DC.BY_NAME["t175"])
    assert t175[2] > 10 * t175[1] > 0
    # the wraps wrap: every word of wrap_all is the model's minus one, the hottest word of wrap_word passes 2^32
    plain = DC.expected(DC.BY_NAME["partial"])[0]
    assert np.array_equal(DC.expected(DC.BY_NAME["wrap_all"])[0], (plain.astype(np.int64) - 1) % 2 ** 32)
    wide = DC.expected(DC.BY_NAME["wide"])[0]
    word = DC.expected(DC.BY_NAME["wrap_word"])[0].ravel()[DC.WRAP_WORD]
    assert int(wide.ravel()[DC.WRAP_WORD]) == int(wide.max()) > 16 and int(word) == int(wide.max()) - 16
    # the band-loop views cross their band limit once, whichever build runs them
    for per_sample in (4, 8):
        (_, rows, rw), (_, cols, cw) = DC.band_views(per_sample, L.MBK_RENDER_BAND_BYTES)
        limit = (L.MBK_RENDER_BAND_BYTES - 1024) // per_sample
        assert limit < rows.width * rows.height <= 2 * limit and limit < cols.width <= 2 * limit and cols.height == 1
        assert all(w[2] * w[3] <= limit for w in rw + cw)
    assert DC.band_views(4, L.MBK_RENDER_BAND_BYTES)[0][1].height == 8200 and DC.band_views(8, L.MBK_RENDER_BAND_BYTES)[0][1].height == 4100


def _edge_restatement(target_name):
    """Where the 81 points z_0 = (i / 4 - 1, j / 4 - 1) of NINE fall, in integers: the cells of EDGE are 1/4 wide and start at
    -1, so z_0 is the lower left corner of cell (i, j); HALF starts half a cell lower, so z_0 is the centre of cell (i, j).
    Either way column 8 and row 8 are outside: on the right and the top edge of EDGE, half a cell beyond those of HALF."""
    import density_cases as DC
    n = DC.view_counts(DC.NINE, 2)
    table = np.zeros((8, 8), np.uint32)
    table[:, :] = (n[:8, :8] == 1)
    return table, int((n == 1).sum()) - int(table.sum())


@pytest.mark.parametrize("name", ["edge", "edge_half", "edge_orbits", "edge_half_orbits"])
def test_table_edges_on_the_host_twin(name):
    """A point exactly on the right or the top edge is outside; row 0 is the lowest imaginary part."""
    import density_cases as DC
    case = DC.BY_NAME[name]
    want, dep, drop, _ = DC.expected(case)
    got, ds = density_host(case.view, case.target, case.mrd, min_count=case.min_count, max_count=case.max_count)
    assert np.array_equal(got, want) and (ds.deposits, ds.dropped) == (dep, drop)
    if case.mrd == 2:
        table, dropped = _edge_restatement(name)
        assert np.array_equal(got, table) and ds.dropped == dropped > 0
        n = DC.view_counts(DC.NINE, 2)
        assert (n[:, 8] == 1).all() and (n[8, 6:] == 1).all()                # samples on the right and on the top edge ...
        assert got[0, 6] == 1 and got[0, 7] == 1 and not got[7, :7].any()    # ... and row 0 holds those with c_i = -1
