"""CPU tests of adaptive supersampling (include/mbk.h, "Adaptive supersampling"): the difference, the decision, the colour and
the resolve the classify and refine kernels are compiled from, run on the host through mbk_render_adaptive_host, against the
numpy restatement of the contract (tests/adaptive_model.py) on synthetic samples."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as A
import render_model as M
from distributedmandelbrot_amd import Palette
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import render_adaptive_host

NEW_SYMBOLS = ["mbk_view_render_adaptive_launch", "mbk_view_render_adaptive_compute", "mbk_render_adaptive_host"]
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (13, 9)]      # W x H
THRESHOLDS = (0, 1, 2, 17, 255, 256)


def test_the_new_symbols_bind_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mbk_abi_version() == 5


def _palette(rs, n=64):
    # scale 1, offset 0: integer nu land exactly on the palette's entries, n - 1 + x on the seam back to entry 0
    return Palette(rs.randint(0, 256, (n, 4)).astype(np.uint8), inside=tuple(int(x) for x in rs.randint(0, 256, 4)),
                   scale=1.0, offset=0.0)


def _samples(rs, h, w, n):
    """Counts a sixth of which (and at least one) are 0; nu in slowly varying patches (so that middle thresholds split the
    pixels), with -inf, exact integers (f = 0), one 256th short of an integer (f = 255) and the wrap k = n - 1 sprinkled in."""
    counts = (rs.randint(0, 6, (h, w)) * rs.randint(1, 5000, (h, w))).astype(np.int32)
    if counts.size > 1:
        counts.flat[rs.randint(0, counts.size)] = 0
    nu = np.cumsum(rs.uniform(-0.02, 0.05, (h, w)), axis=1) + rs.uniform(0.0, 3.0 * n)
    kind = rs.randint(0, 12, (h, w))
    nu = np.where(kind == 0, -np.inf, nu)
    nu = np.where(kind == 1, np.floor(nu), nu)
    nu = np.where(kind == 2, np.floor(nu) + 255.0 / 256.0, nu)
    nu = np.where(kind == 3, float(n - 1) + 0.5 + n * rs.randint(0, 9, (h, w)), nu)
    return counts, nu.astype(np.float64)


@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("w, h", SHAPES + [(40, 28)])
def test_window_form_of_the_model_equals_the_whole_view_form(w, h, s):
    """adaptive_model.render_adaptive_window (the window's fine samples and a one-pixel halo of the base samples) against
    render_adaptive of the whole view, on the synthetic samples of the twin's test: the whole view as a window, every corner,
    every edge, single pixels at the last column and row, and an interior window."""
    rs = np.random.RandomState(1000 * s + 17 * w + h)
    pal = _palette(rs)
    bc, bn = _samples(rs, h, w, len(pal))
    fc, fn = _samples(rs, h * s, w * s, len(pal))
    windows = {(0, 0, w, h), (w - 1, h - 1, 1, 1), (0, 0, 1, 1), (w - 1, 0, 1, h), (0, h - 1, w, 1), (0, 0, (w + 1) // 2, (h + 1) // 2),
               (w // 2, h // 2, w - w // 2, h - h // 2), (w // 3, h // 3, max(w // 3, 1), max(h // 3, 1))}
    for thr in THRESHOLDS:
        want, want_mask = A.render_adaptive(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, bc, bn, fc, fn)
        for window in windows:
            c0, r0, nc, nr = window
            hc0, hr0, hnc, hnr = A.halo(window, w, h)
            got, mask = A.render_adaptive_window(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, window, w, h,
                                                 bc[hr0:hr0 + hnr, hc0:hc0 + hnc], bn[hr0:hr0 + hnr, hc0:hc0 + hnc],
                                                 fc[r0 * s:(r0 + nr) * s, c0 * s:(c0 + nc) * s], fn[r0 * s:(r0 + nr) * s, c0 * s:(c0 + nc) * s])
            assert np.array_equal(got, want[r0:r0 + nr, c0:c0 + nc]) and np.array_equal(mask, want_mask[r0:r0 + nr, c0:c0 + nc]), (thr, window)


@pytest.mark.parametrize("s", M.SUPERSAMPLES)
@pytest.mark.parametrize("w, h", SHAPES)
def test_twin_equals_the_model_on_synthetic_samples(w, h, s):
    rs = np.random.RandomState(1000 * s + 17 * w + h)
    pal = _palette(rs)
    bc, bn = _samples(rs, h, w, len(pal))
    fc, fn = _samples(rs, h * s, w * s, len(pal))
    assert ((bc == 0).any() and (bc != 0).any()) or w * h < 3
    full = M.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, s, fc, fn)
    base = M.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, 1, bc, bn)
    for thr in THRESHOLDS:
        got, mask = render_adaptive_host(pal, s, thr, w, h, base_counts=bc, base_smooth=bn, fine_counts=fc, fine_smooth=fn,
                                         want_mask=True)
        want, want_mask = A.render_adaptive(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, bc, bn, fc, fn)
        assert np.array_equal(got, want), (thr, int((got != want).any(axis=2).sum()))
        assert np.array_equal(mask, want_mask), thr
        # without a mask: the same image
        assert np.array_equal(render_adaptive_host(pal, s, thr, w, h, base_counts=bc, base_smooth=bn, fine_counts=fc,
                                                   fine_smooth=fn), got)
        if thr == 0:
            assert mask.all() and np.array_equal(got, full)
        if thr == 256:
            assert not mask.any() and np.array_equal(got, base)


def test_middle_thresholds_split_the_pixels():
    """The synthetic samples are not all-or-nothing: at 13 x 9 some threshold refines some pixels and leaves others."""
    rs = np.random.RandomState(7)
    pal = _palette(rs)
    bc, bn = _samples(rs, 9, 13, len(pal))
    base = A.base_image(pal.entries, pal.inside, pal.scale, pal.offset, bc, bn)
    shares = [A.refined_mask(base, t).mean() for t in (2, 17, 255)]
    assert any(0.0 < x < 1.0 for x in shares), shares


def _flat_case(delta, channel, thr, s=2, w=6, h=5):
    """An image whose base colours are all (100, 100, 100, 100) except the corner pixel (0, 0), whose `channel` is 100 + delta;
    the fine samples give every pixel (7, 7, 7, 7).  Returns (rgba, mask)."""
    entries = np.full((4, 4), 100, np.uint8)
    entries[1, channel] = 100 + delta
    entries[2] = 7
    pal = Palette(entries, inside=(0, 0, 0, 0), scale=1.0, offset=0.0)
    bc = np.ones((h, w), np.int32)
    bn = np.zeros((h, w), np.float64)
    bn[0, 0] = 1.0                                   # entry 1 exactly (f = 0)
    fc = np.ones((h * s, w * s), np.int32)
    fn = np.full((h * s, w * s), 2.0)
    return render_adaptive_host(pal, s, thr, w, h, base_counts=bc, base_smooth=bn, fine_counts=fc, fine_smooth=fn,
                                want_mask=True)


@pytest.mark.parametrize("channel", [0, 1, 2, 3])     # 3: a difference in alpha only
@pytest.mark.parametrize("thr", [1, 17, 155])
def test_a_corner_pixel_exactly_at_the_threshold_is_refined_with_its_three_neighbours(thr, channel):
    rgba, mask = _flat_case(thr, channel, thr)
    want = np.zeros_like(mask)
    want[0:2, 0:2] = 1
    assert np.array_equal(mask, want)
    assert (rgba[0:2, 0:2] == 7).all()
    assert (rgba[mask == 0] == 100).all()
    if thr > 1:
        rgba, mask = _flat_case(thr - 1, channel, thr)
        assert not mask.any()
        corner = [100, 100, 100, 100]
        corner[channel] += thr - 1
        assert tuple(rgba[0, 0]) == tuple(corner) and (rgba.reshape(-1, 4)[1:] == 100).all()


def _spec(source=L.MBK_RENDER_SMOOTH, s=2, pal=None, n=None):
    pal = np.zeros((2, 4), np.uint8) if pal is None else pal
    return L.mbk_render_spec(source, s, pal.ctypes.data, len(pal) if n is None else n, (C.c_uint8 * 4)(0, 0, 0, 255), 1.0, 0.0,
                             0), pal


def test_the_twin_refuses_bad_arguments_and_writes_nothing():
    lib = L.load()
    w, h, s = 4, 3, 2
    bc, bn = np.ones((h, w), np.int32), np.ones((h, w), np.float64)
    fc, fn = np.ones((h * s, w * s), np.int32), np.ones((h * s, w * s), np.float64)

    def call(spec, thr=17, width=w, height=h, arrs=(bc, bn, fc, fn), out=True):
        rgba = np.full((h, w, 4), 0xA5, np.uint8)
        mask = np.full((h, w), 0xA5, np.uint8)
        st = lib.mbk_render_adaptive_host(C.byref(spec) if spec is not None else None, thr, width, height,
                                          *[a.ctypes.data if a is not None else None for a in arrs],
                                          rgba.ctypes.data if out else None, mask.ctypes.data)
        assert st == L.MBK_OK or ((rgba == 0xA5).all() and (mask == 0xA5).all())
        return st

    ok, _keep = _spec()
    assert call(ok) == L.MBK_OK and call(ok, thr=256) == L.MBK_OK and call(ok, thr=0) == L.MBK_OK
    assert call(ok, thr=257) == L.MBK_ERR_INVALID
    assert call(ok, thr=2 ** 32 - 1) == L.MBK_ERR_INVALID
    for source, pal in ((L.MBK_RENDER_BYTES, np.zeros((256, 4), np.uint8)), (L.MBK_RENDER_DISTANCE, None),
                        (L.MBK_RENDER_DISTANCE_REL, None), (L.MBK_RENDER_EQUALIZED, None), (7, None)):
        spec, _k = _spec(source=source, pal=pal)
        assert call(spec) == L.MBK_ERR_INVALID, source
    assert call(None) == L.MBK_ERR_INVALID
    assert call(ok, out=False) == L.MBK_ERR_INVALID
    for k in range(4):
        arrs = [bc, bn, fc, fn]
        arrs[k] = None
        assert call(ok, arrs=arrs) == L.MBK_ERR_INVALID, k
    nopal = L.mbk_render_spec(L.MBK_RENDER_SMOOTH, 2, None, 2, (C.c_uint8 * 4)(0, 0, 0, 255), 1.0, 0.0, 0)
    assert call(nopal) == L.MBK_ERR_INVALID
    for bad_s in (0, 5, 16):
        spec, _k = _spec(s=bad_s)
        assert call(spec) == L.MBK_ERR_INVALID, bad_s
    assert call(ok, width=0) == L.MBK_ERR_INVALID and call(ok, height=0) == L.MBK_ERR_INVALID
    assert call(ok, width=2 ** 30) == L.MBK_ERR_INVALID
