"""The case table of the density-view GPU tests (include/mbk.h, "Density views"), shared by the plain build's tests
(tests/test_gpu_density.py) and the compact build's (tests/test_gpu_density_compact.py through tests/density_child.py), with
the two helpers both need: `expected`, the table a case must produce according to tests/density_model.py, and `run_case`,
the case on a device.  Not a test module, and not a conftest.

The shapes are the smallest at which the list kernels of the compact replay (csrc/mbk_density.h) can go wrong; what each one
reaches is said beside it.  tests/test_density.py checks on the CPU that the cases are what they claim to be.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

import density_model as M

from distributedmandelbrot_amd import DensityTarget, View

GUARD = 0xA5A5A5A5
GUARD_WORDS = 256

VIEW = View(-2.0, -1.25, 3.0, 2.5, 96, 64)
MRD = 200
WIDE = DensityTarget(-2.0, -1.5, 3.0, 3.0, 48, 40)
NARROW = DensityTarget(-0.5, 0.5, 0.5, 0.5, 48, 40)     # [-0.5, 0] x [0.5, 1]: most points miss it
DISC = DensityTarget(-2.5, -2.5, 5.0, 5.0, 40, 40)      # contains the disc of radius 2
BIG = View(-2.0, -1.25, 3.0, 2.5, 100, 70)
SMALL = View(-2.0, -1.25, 3.0, 2.5, 13, 9)
ENDS = View(-2.0, -1.25, 3.0, 2.5, 40, 24)
INNER = View(-1.9, -1.2, 2.4, 2.4, 48, 40)              # inside DISC, and |c| <= 2.25 < 2.5
FAR = View(-3.0, 2.5, 0.25, 0.25, 16, 16)               # |c| > 3.9: every sample has n = 1
FAR_TARGET = DensityTarget(-3.25, 2.25, 0.75, 0.75, 12, 12)
T11 = DensityTarget(-2.5, -2.5, 5.0, 5.0, 1, 1)
T22 = DensityTarget(-2.5, -2.5, 5.0, 5.0, 2, 2)
T175 = DensityTarget(-0.3, 0.55, 0.31, 0.2, 17, 5)      # most points fall outside it
# Table edges: the 9 x 9 samples are k / 4 - 1, binary fractions, and the cells of EDGE are 1/4 wide, so every z_0 lies exactly
# on a cell corner, column 8 and row 8 exactly on the right and the top edge.  HALF is EDGE moved by half a cell: no z_0 on an edge.
NINE = View(-1.0, -1.0, 2.0, 2.0, 9, 9)
EDGE = DensityTarget(-1.0, -1.0, 2.0, 2.0, 8, 8)
HALF = DensityTarget(-1.125, -1.125, 2.0, 2.0, 8, 8)
INTERIOR_WINDOW = (48, 20, 8, 8)                        # of VIEW: inside the main cardioid, no sample escapes
SPARSE_WINDOW = (40, 20, 8, 8)                          # of VIEW: across the cardioid's edge, 20 samples escape -- under one wave
WRAP_WORD = 19 * 48 + 10                                # the cell of WIDE that VIEW's orbits reach most often, 78 times
BAND_TARGET = DensityTarget(-2.5, -2.5, 5.0, 5.0, 512, 512)
BAND_MRD = 8


class Case(NamedTuple):
    name: str
    view: View
    windows: Tuple[Optional[Tuple[int, int, int, int]], ...]   # one launch each; None: the whole view
    target: DensityTarget
    mrd: int
    min_count: int
    max_count: int
    entry: str                  # "compute": compute_view_density (one window); "launch": launch_view_density into a guarded table
    init: Tuple = ()            # launch: what the table holds before: () zeros, ("all", v) or ("word", index, v)


def _c(name, view, target, mrd=MRD, lo=1, hi=0, windows=(None,), entry="compute", init=()):
    return Case(name, view, tuple(windows), target, mrd, lo, hi, entry, init)


CASES = (
    # bands 0 to 7 populated, the list longer than one 256-thread workgroup
    _c("wide", VIEW, WIDE), _c("narrow", VIEW, NARROW),
    # 117 samples: a partial workgroup in the two list passes, a last wave of fewer than 64 entries
    _c("partial", SMALL, WIDE),
    # every qualifying sample has n = 1, then n in {1, 2}: band 0 alone, then bands 0 and 1
    _c("mrd2", ENDS, WIDE, 2), _c("mrd3", ENDS, WIDE, 3), _c("mrd258", ENDS, WIDE, 258),
    _c("mrd2_top", ENDS, WIDE, 2, 1, 1), _c("mrd3_top", ENDS, WIDE, 3, 2, 2), _c("mrd258_top", ENDS, WIDE, 258, 257, 257),
    # n = 2^k - 1 against 2^k at a band boundary; a filter that empties every band but one
    _c("n255_256", ENDS, WIDE, 258, 255, 256), _c("n256_257", ENDS, WIDE, 258, 256, 257), _c("n128", ENDS, WIDE, 258, 128, 128),
    # ... and the same filters where the view has such samples (VIEW's 6144 samples hold n = 7, 8, 15, 16, 31, 32)
    _c("n7_8", VIEW, WIDE, 258, 7, 8), _c("n8_9", VIEW, WIDE, 258, 8, 9), _c("n15_16", VIEW, WIDE, 258, 15, 16),
    _c("n31_32", VIEW, WIDE, 258, 31, 32), _c("n16", VIEW, WIDE, 258, 16, 16), _c("n128_view", VIEW, WIDE, 258, 128, 128),
    # no sample qualifies: total = 0, every replay wave returns after its loads
    _c("interior", VIEW, WIDE, windows=(INTERIOR_WINDOW,)),
    # a list shorter than one wave
    _c("sparse", VIEW, WIDE, windows=(SPARSE_WINDOW,)),
    # every sample has n = 1: the list equals the window
    _c("far", FAR, FAR_TARGET),
    # nothing is deposited
    _c("mrd0", ENDS, WIDE, 0), _c("mrd1", ENDS, WIDE, 1),
    # launches add up, the band words are cleared per launch
    _c("big_whole", BIG, WIDE, entry="launch"),
    _c("big_rows", BIG, WIDE, windows=((0, 0, 100, 23), (0, 23, 100, 24), (0, 47, 100, 23)), entry="launch"),
    _c("big_cols", BIG, WIDE, windows=((0, 0, 9, 70), (9, 0, 41, 70), (50, 0, 49, 70), (99, 0, 1, 70)), entry="launch"),
    _c("big_once", BIG, WIDE, windows=((17, 11, 30, 21),), entry="launch"),
    _c("big_twice", BIG, WIDE, windows=((17, 11, 30, 21), (17, 11, 30, 21)), entry="launch"),
    # contention: one hot address, four
    _c("one_cell", INNER, T11), _c("four_cells", INNER, T22, entry="launch"),
    # most points fall outside the table: nothing is written around it
    _c("t175", VIEW, T175, entry="launch"),
    # a launch adds modulo 2^32
    _c("wrap_all", SMALL, WIDE, entry="launch", init=("all", 0xFFFFFFFF)),
    _c("wrap_word", VIEW, WIDE, entry="launch", init=("word", WRAP_WORD, 0xFFFFFFF0)),
    # the right and the top edge are outside, row 0 is the lowest imaginary part; mrd 2, n = 1: z_0 alone is deposited
    _c("edge", NINE, EDGE, 2, 1, 1, entry="launch"), _c("edge_half", NINE, HALF, 2, 1, 1, entry="launch"),
    _c("edge_orbits", NINE, EDGE, 50, entry="launch"), _c("edge_half_orbits", NINE, HALF, 50, entry="launch"),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def initial(case: Case) -> np.ndarray:
    """The words of the table before the case's launches."""
    table = np.zeros(case.target.width * case.target.height, np.uint32)
    if case.init:
        if case.init[0] == "all":
            table[:] = case.init[1]
        else:
            table[case.init[1]] = case.init[2]
    return table


_counts = {}


def view_counts(view, mrd) -> np.ndarray:
    """The model's counts of a whole view, computed once per (view, mrd)."""
    key = (view, int(mrd))
    if key not in _counts:
        xs, ys = M.axes(view)
        cr, ci = np.meshgrid(xs, ys)
        n = M.counts(cr, ci, mrd)
        n.setflags(write=False)
        _counts[key] = n
    return _counts[key]


def expected(case: Case):
    """(table uint32[H, W], deposits, dropped, qualifying n of every launch concatenated) by the model: the launches added to
    the initial table modulo 2^32."""
    full = view_counts(case.view, case.mrd)
    total = np.zeros((case.target.height, case.target.width), np.uint64)
    deposits = dropped = 0
    ns = []
    for window in case.windows:
        col0, row0, ncols, nrows = window if window is not None else (0, 0, case.view.width, case.view.height)
        n = full[row0:row0 + nrows, col0:col0 + ncols]
        table, dep, drop, _ = M.accumulate(case.view, case.target, case.mrd, case.min_count, case.max_count, window=window, n=n)
        total += table
        deposits += dep
        dropped += drop
        ns.append(n[M.qualify(n, case.mrd, case.min_count, case.max_count)])
    total += initial(case).reshape(total.shape)
    return (total & 0xFFFFFFFF).astype(np.uint32), deposits, dropped, np.concatenate(ns)


def device_table(gpu, view, target, mrd, launches, guard=GUARD_WORDS, init=None, **kw):
    """The table after `launches` (a list of windows, None = the whole view) into one device table -- cleared, or holding the
    words `init` -- with `guard` sentinel words on either side.  Returns (table, sentinels intact, the device buffer)."""
    import torch
    cells = target.width * target.height
    host = np.full(cells + 2 * guard, GUARD, np.uint32)
    host[guard:guard + cells] = 0 if init is None else init
    buf = torch.from_numpy(host.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    for window in launches:
        gpu.launch_view_density(view, target, mrd, d_density=buf.data_ptr() + 4 * guard, window=window, **kw)
    torch.cuda.synchronize()
    back = buf.cpu().numpy().view(np.uint32)
    intact = bool((back[:guard] == GUARD).all() and (back[guard + cells:] == GUARD).all())
    return back[guard:guard + cells].reshape(target.height, target.width), intact, buf


def run_case(gpu, case: Case) -> dict:
    """The case on the device: its table; deposits and dropped ("compute"); the sentinels and mbk_density_max of the device
    table ("launch")."""
    if case.entry == "compute":
        table, st, ds = gpu.compute_view_density(case.view, case.target, case.mrd, min_count=case.min_count, max_count=case.max_count,
                                                 window=case.windows[0])
        return {"table": table, "deposits": ds.deposits, "dropped": ds.dropped, "never": st.never_pixels}
    table, intact, buf = device_table(gpu, case.view, case.target, case.mrd, case.windows, init=initial(case),
                                      min_count=case.min_count, max_count=case.max_count)
    mx, total = gpu.density_max(buf.data_ptr() + 4 * GUARD_WORDS, table.size)
    return {"table": table, "intact": intact, "max": mx, "total": total}


def check_case(case: Case, got: dict) -> None:
    """`got` (run_case) against the model, exactly."""
    want, dep, drop, _ = expected(case)
    assert got["table"].dtype == np.uint32 and np.array_equal(got["table"], want), case.name
    if case.entry == "compute":
        assert (int(got["deposits"]), int(got["dropped"])) == (dep, drop), case.name
        col0, row0, ncols, nrows = case.windows[0] if case.windows[0] is not None else (0, 0, case.view.width, case.view.height)
        n = view_counts(case.view, case.mrd)[row0:row0 + nrows, col0:col0 + ncols]
        assert int(got["never"]) == int((n == 0).sum()), case.name
    else:
        assert got["intact"], f"{case.name}: a word outside the table was written"
        assert (int(got["max"]), int(got["total"])) == (int(want.max()), int(want.astype(np.uint64).sum())), case.name


# ---- the band loop of density_run (csrc/mbk_api.hip): views of more samples than one band of the count scratch holds ------

def band_views(per_sample: int, band_bytes: int):
    """[(name, view, the same view as two windows, each below the band limit)] for a build that keeps `per_sample` bytes of
    scratch per sample: a view of two row bands, and one row too wide for a band, cut into two column tiles."""
    budget = band_bytes - 1024
    limit = budget // per_sample                 # samples to a band: 67 108 608 plain, 33 554 304 compact
    w = 8192
    h, n = {4: (8200, 67110000), 8: (4100, 33556000)}[per_sample]
    band_rows = budget // (w * per_sample)       # 8191 plain, 4095 compact
    rows = View(-2.0, -1.25, 2.5, 2.5, w, h)
    cols = View(-2.0, 0.3, 2.5, 1.0, n, 1)
    assert band_rows < h <= 2 * band_rows and w * (h // 2) <= limit < w * h      # two row bands; each half is one
    assert limit < n <= 2 * limit and n // 2 <= limit                            # two column tiles; each half is one
    return [("rows", rows, ((0, 0, w, h // 2), (0, h // 2, w, h - h // 2))), ("cols", cols, ((0, 0, n // 2, 1), (n // 2, 0, n - n // 2, 1)))]


def run_band_view(gpu, view, windows) -> dict:
    """One view at BAND_MRD into BAND_TARGET: through compute_view_density, and as two window launches into one device table."""
    table, st, ds = gpu.compute_view_density(view, BAND_TARGET, BAND_MRD)
    two, intact, _ = device_table(gpu, view, BAND_TARGET, BAND_MRD, windows)
    return {"table": table, "two": two, "intact": intact, "deposits": ds.deposits, "dropped": ds.dropped,
            "never": st.never_pixels, "pixel_iterations": st.pixel_iterations, "kernel_ms": st.kernel_ms}


def check_band_view(oracle, view, got: dict) -> None:
    """`got` (run_band_view) against the host twin's table -- held to the model bit for bit at small shapes by
    tests/test_density.py -- and the C oracle's statistics of the same view."""
    from distributedmandelbrot_amd.device import density_host
    host, hs = density_host(view, BAND_TARGET, BAND_MRD)
    oc, _, total = oracle.view(view.start_r, view.start_i, view.range_r, view.range_i, view.width, view.height, BAND_MRD, want_bytes=False)
    never = int(oc.size - np.count_nonzero(oc))
    del oc
    assert got["intact"], "a word outside the table was written"
    assert np.array_equal(got["table"], host) and np.array_equal(got["two"], host)
    assert (int(got["pixel_iterations"]), int(got["never"])) == (total, never)
    assert (int(got["deposits"]), int(got["dropped"])) == (hs.deposits, hs.dropped)
    assert hs.deposits + hs.dropped == total - (BAND_MRD - 1) * never and hs.dropped == 0 and hs.deposits == int(host.sum(dtype=np.uint64))
