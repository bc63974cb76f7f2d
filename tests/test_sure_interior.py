"""MBK_OPT_SURE_INTERIOR on the host (include/mbk.h; csrc/mbk_kernels.h sure_interior_point, block_pixel): the certificate
that sends a block of the interior class to the test-free loop, the count of the blocks it certifies, and the word a launch
carries.  The kernels never trust the certificate (a block whose final test trips is computed again), so what is checked here is
that it predicts well: it accepts no pixel that escapes -- every acceptance of an escaping pixel would cost a replay -- and it
accepts most of the pixels that do not."""
import ctypes as C

import numpy as np
import pytest

CFG2 = (-2.0, -1.5, 3.0, 3.0)          # BASELINE cfg2: the full set, centre -0.5 + 0i, span 3
INSET = (-0.2, -0.1, 0.2, 0.2)         # bench.py's `inset`: inside the main cardioid
CFG3 = (-0.743648, 0.131820, 1e-5, 1e-5)   # BASELINE cfg3: a deep zoom beside the set (centre -0.743643 + 0.131825i)
ORACLE_MRD = 5000


@pytest.fixture(scope="module")
def lib():
    from distributedmandelbrot_amd import _lib as L
    return L.load()


def _accepted(lib, oracle, start_r, start_i, range_r, range_i, n):
    xs, ys = oracle.axis(start_r, range_r, n), oracle.axis(start_i, range_i, n)
    point = lib.mbk_sure_interior_point
    return np.array([[point(float(x), float(y)) for x in xs] for y in ys], dtype=bool)


@pytest.fixture(scope="module")
def cfg2_1024(lib, oracle):
    """(accepted, oracle counts) of the cfg2 view at 1024 x 1024, computed once."""
    counts, _, _ = oracle.view(*CFG2, 1024, 1024, ORACLE_MRD, want_bytes=False)
    return _accepted(lib, oracle, *CFG2, 1024), counts


def test_accepted_points_never_escape_on_the_full_view(cfg2_1024):
    accepted, counts = cfg2_1024
    assert accepted.any()
    assert not counts[accepted].any()


@pytest.mark.parametrize("centre", [(0.25, 0.0), (-0.75, 0.0), (-1.25, 0.0), (-0.125, 0.65)],
                         ids=["cusp", "contact", "disk_far_end", "cardioid_top"])
def test_accepted_points_never_escape_where_the_margin_is_thin(lib, oracle, centre):
    """256 x 256 windows of span 0.02 on the places where a closed form touches its boundary: the cusp of the cardioid, the point
    where cardioid and disk meet, the far end of the disk, the top of the cardioid."""
    span = 0.02
    view = (centre[0] - span / 2, centre[1] - span / 2, span, span)
    counts, _, _ = oracle.view(*view, 256, 256, ORACLE_MRD, want_bytes=False)
    accepted = _accepted(lib, oracle, *view, 256)
    assert not counts[accepted].any()
    # (none of these windows lies wholly inside or outside: some pixel is refused, and away from the cusp some is accepted)
    assert not accepted.all()
    if centre != (0.25, 0.0):
        assert accepted.any()


def test_coverage_of_the_never_escaping_pixels(cfg2_1024):
    """A certificate that accepts nothing is useless.  The share of the never-escaping pixels it accepts is a ratio of areas
    (0.907 at 4096 x 4096 and mrd 1000)."""
    accepted, counts = cfg2_1024
    never = counts == 0
    share = float((accepted & never).sum()) / float(never.sum())
    print(f"accepted share of the never-escaping pixels: {share:.4f}")
    assert share >= 0.85


def test_the_two_closed_forms_and_the_margin(lib):
    point = lib.mbk_sure_interior_point
    assert point(0.0, 0.0) == 1 and point(-1.0, 0.0) == 1 and point(-0.1, 0.1) == 1
    assert point(0.3, 0.0) == 0 and point(-2.0, 0.0) == 0 and point(-0.75, 0.3) == 0 and point(0.0, 1.0) == 0
    assert point(float("nan"), 0.0) == 0 and point(0.0, float("inf")) == 0
    # the disk (cr + 1)^2 + ci^2 < 1/16 - 1e-4 on the real axis: its radius is sqrt(0.0624) = 0.24980 and not 0.25
    assert point(-1.0 + 0.2497, 0.0) == 1 and point(-1.0 + 0.2499, 0.0) == 0
    assert point(-1.0 - 0.2497, 0.0) == 1 and point(-1.0 - 0.2499, 0.0) == 0


def _blocks(lib, view, n, window=None):
    from distributedmandelbrot_amd import _lib as L
    col0, row0, ncols, nrows = window if window is not None else (0, 0, n, n)
    cv = L.mbk_view(*view, n, n, col0, row0, ncols, nrows)
    out = C.c_uint64(0)
    assert lib.mbk_sure_interior_blocks(C.byref(cv), C.byref(out)) == L.MBK_OK
    return int(out.value)


def test_block_counter(lib, oracle):
    assert _blocks(lib, INSET, 256) > 0
    assert _blocks(lib, (-2.0, -2.0, 1.0, 1.0), 256) == 0
    # against the point function on a view that holds part of the boundary: whole 8x8 blocks, all 64 pixels accepted
    # (the window stops short of the axes' last samples, so every block's coordinates are the regular formula's)
    accepted = _accepted(lib, oracle, *CFG2, 257)[:256, :256]
    want = int(accepted.reshape(32, 8, 32, 8).all(axis=(1, 3)).sum())
    assert want > 0 and _blocks(lib, CFG2, 257, (0, 0, 256, 256)) == want


def _flag(lib, view, n, mrd, *, f32=False, cyc=0, option=1):
    from distributedmandelbrot_amd import _lib as L
    cv = L.mbk_view(*view, n, n, 0, 0, n, n)
    out = C.c_uint32(99)
    assert lib.mbk_sure_interior_flag(C.byref(cv), mrd, L.MBK_PRECISION_F32 if f32 else 0, cyc, option, C.byref(out)) == L.MBK_OK
    return int(out.value)


def test_host_flag(lib):
    assert _flag(lib, CFG2, 4096, 1000) == 1
    assert _flag(lib, CFG2, 1024, 130) == 1 and _flag(lib, INSET, 256, 65) == 1
    assert _flag(lib, CFG3, 8192, 10000) == 0          # a deep zoom does not pay for the certificate
    assert _flag(lib, (-2.0, -2.0, 1.0, 1.0), 4096, 1000) == 0   # nor does an all-exterior tile
    assert _flag(lib, CFG2, 4096, 1000, cyc=1) == 0
    assert _flag(lib, CFG2, 4096, 1000, f32=True) == 0
    assert _flag(lib, CFG2, 4096, 32) == 0 and _flag(lib, CFG2, 4096, 64) == 0
    assert _flag(lib, CFG2, 4096, 1000, option=0) == 0
    # force mode ignores the window, not the kind of launch
    assert _flag(lib, CFG3, 8192, 10000, option=2) == 2 and _flag(lib, CFG2, 4096, 1000, option=2) == 2
    assert _flag(lib, CFG2, 4096, 1000, option=2, cyc=1) == 0 and _flag(lib, CFG2, 4096, 32, option=2) == 0
