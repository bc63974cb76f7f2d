"""MBK_OPT_SURE_INTERIOR on the device (include/mbk.h; csrc/mbk_kernels.h block_pixel, csrc/mbk_loops.inc escape_steps_sure):
blocks of the interior class that a closed-form certificate accepts run their steps without bailout tests and are tested once
at the end; a wave whose test trips computes its block again the usual way.  The option may change how long a launch takes and
nothing else: every test here compares the outputs byte for byte across option 0 (off), 1 (on) and 2 (force: every block of the
interior class takes the test-free loop, so the fallback is reached), and against the C oracle."""
import ctypes as C

import numpy as np
import pytest

from distributedmandelbrot_amd import View
from distributedmandelbrot_amd import _lib as L

pytestmark = pytest.mark.gpu

INSET = View(-0.2, -0.1, 0.2, 0.2, 256, 256)           # bench.py's `inset` at 256 x 256: every pixel inside the main cardioid
EDGE = View(-0.78, 0.05, 0.08, 0.08, 256, 256)         # over the cardioid's edge beside the period-2 disk
CFG2 = View(-2.0, -1.5, 3.0, 3.0, 1024, 1024)          # the full set; 16 384 blocks: the smallest launch the units kernel serves
CONTACT = View(-0.775, -0.025, 0.05, 0.05, 512, 512)   # holds -0.75, where cardioid and disk touch and both closed forms nearly hold


@pytest.fixture
def dev(gpu):
    saved = {k: gpu.get_option(k) for k in ("sure_interior", "cycle_detect")}
    gpu.set_option("cycle_detect", 0)
    yield gpu
    for k, v in saved.items():
        gpu.set_option(k, v)


def _host(view, mrd, cyc=0, option=1):
    """(certified blocks, the launch's word) from the host twins."""
    cv = L.mbk_view(view.start_r, view.start_i, view.range_r, view.range_i, view.width, view.height, 0, 0, view.width, view.height)
    lib = L.load()
    n, w = C.c_uint64(0), C.c_uint32(99)
    assert lib.mbk_sure_interior_blocks(C.byref(cv), C.byref(n)) == L.MBK_OK
    assert lib.mbk_sure_interior_flag(C.byref(cv), mrd, 0, cyc, option, C.byref(w)) == L.MBK_OK
    return int(n.value), int(w.value)


def _oracle(oracle, view, mrd):
    return oracle.view(view.start_r, view.start_i, view.range_r, view.range_i, view.width, view.height, mrd)


def _compute(dev, view, mrd, option, **kw):
    dev.set_option("sure_interior", option)
    return dev.compute_view(view, mrd, kernel="group", **kw)


def _check_outputs(dev, view, mrd, oc, ob, total, options=(0, 1, 2)):
    """counts, bytes, both, and bytes with the statistics fused (no counts wanted), under every option."""
    never = int((oc == 0).sum())
    for option in options:
        c, b, st = _compute(dev, view, mrd, option)
        assert np.array_equal(c, oc) and np.array_equal(b, ob), (mrd, option, "both")
        assert st.pixel_iterations == total and st.never_pixels == never, (mrd, option, "both")
        c, _, st = _compute(dev, view, mrd, option, want_bytes=False)
        assert np.array_equal(c, oc) and st.pixel_iterations == total and st.never_pixels == never, (mrd, option, "counts")
        _, b, st = _compute(dev, view, mrd, option, want_counts=False)
        assert np.array_equal(b, ob), (mrd, option, "bytes")
        assert st.pixel_iterations == total and st.never_pixels == never, (mrd, option, "bytes + statistics")


@pytest.mark.parametrize("mrd", [65, 66, 96, 97, 98, 129])
def test_remainders_and_trip_boundary(dev, oracle, mrd):
    """mrd - 1 = 64, 65, 95, 96, 97, 128 steps: whole 32-step trips only, one single step, 31 of them, and the trip boundary from
    both sides.  Every block of the view is certified (the host counter says so), so with option 1 every block takes the
    test-free loop and none the fallback; at 1 024 blocks the launch is tile_asm_kernel's, in image order."""
    assert _host(INSET, mrd) == (1024, 1)
    oc, ob, total = _oracle(oracle, INSET, mrd)
    assert not oc.any()
    _check_outputs(dev, INSET, mrd, oc, ob, total)


def test_fallback(dev, oracle):
    """A window over the set's edge under force mode: blocks that hold escaping pixels run the test-free loop, trip its final test
    and are computed again.  Counts, bytes, both and the smooth output equal option 0's, the smooth values bit for bit."""
    mrd = 300
    certified, word = _host(EDGE, mrd, option=2)
    assert 0 < certified < 1024 and word == 2
    oc, ob, total = _oracle(oracle, EDGE, mrd)
    escaping_blocks = int((oc.reshape(32, 8, 32, 8) > 0).any(axis=(1, 3)).sum())
    assert escaping_blocks > 100          # the fallback has work to do
    _check_outputs(dev, EDGE, mrd, oc, ob, total)
    smooth = {}
    for option in (0, 1, 2):
        dev.set_option("sure_interior", option)
        s, c, _ = dev.compute_view_smooth(EDGE, mrd, kernel="group")
        assert np.array_equal(c, oc), option
        smooth[option] = s
    assert (smooth[0][oc > 0] > 0).all() and not smooth[0][oc == 0].any()
    for option in (1, 2):
        assert np.array_equal(smooth[option].view(np.uint64), smooth[0].view(np.uint64)), option


def test_units_kernel(dev, oracle):
    """The full set at 1024 x 1024: 16 384 blocks, the smallest launch the units kernel serves (its heavy list is the interior
    class).  Counts, bytes, both, and bytes with the statistics fused into the kernel."""
    mrd = 130
    certified, word = _host(CFG2, mrd)
    assert certified > 2000 and word == 1
    oc, ob, total = _oracle(oracle, CFG2, mrd)
    _check_outputs(dev, CFG2, mrd, oc, ob, total)


def test_contact_point(dev, oracle):
    mrd = 200
    certified, word = _host(CONTACT, mrd)
    assert 0 < certified < 4096 and word == 1
    oc, ob, total = _oracle(oracle, CONTACT, mrd)
    assert (oc > 0).any() and (oc == 0).any()
    _check_outputs(dev, CONTACT, mrd, oc, ob, total)


@pytest.mark.parametrize("view,mrd", [(INSET, 129), (EDGE, 300), (CFG2, 130)], ids=["inset", "edge", "cfg2"])
def test_cycle_test_on(dev, oracle, view, mrd):
    """With the cycle test the launch carries no word and the path is not taken: options 0 and 1 give the same outputs."""
    assert _host(view, mrd, cyc=1)[1] == 0
    dev.set_option("cycle_detect", 1)
    oc, ob, total = _oracle(oracle, view, mrd)
    never = int((oc == 0).sum())
    for option in (0, 1):
        c, b, st = _compute(dev, view, mrd, option)
        assert np.array_equal(c, oc) and np.array_equal(b, ob), option
        assert st.pixel_iterations == total and st.never_pixels == never, option
