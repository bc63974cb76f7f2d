"""CPU tests of adaptive supersampling of deep views (include/mbk.h, the section of that name): the new entry points bind, the
shared cases (tests/deep_adaptive_cases.py) are what the GPU tests need them to be -- middle thresholds that refine neither
nothing nor everything, shapes whose base and fine views need two bilinear-approximation tables and one whose views share
one --, and the host contract stays blind to the kind of view its samples come from."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_model as A
import deep_adaptive_cases as K
import deep_bla_model as B
from distributedmandelbrot_amd import MandelbrotDevice
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import render_adaptive_host

NEW_SYMBOLS = ["mbk_deep_view_render_adaptive_launch", "mbk_deep_view_render_adaptive_compute"]
GPU_SUPERSAMPLES = (2, 3, 4, 8)      # render_model.SUPERSAMPLES past 1, which has no finer view

# the refined share of the model's mask at the middle threshold on the library's orbit table, W x H (test 2 prints them)
SHARES = {"i-30": 0.135, "i-30-two-tables": 0.157, "i-200-two-tables": 0.305, "M58": 0.200, "seahorse": 0.246}


def test_the_new_symbols_bind_and_refuse_a_null_ctx():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mbk_abi_version() == 5
    for name in ("render_deep_view_adaptive", "launch_render_deep_view_adaptive"):
        assert callable(getattr(MandelbrotDevice, name))
    out = np.full(16, 0xA5, np.uint8)
    assert lib.mbk_deep_view_render_adaptive_launch(None, None, None, 100, 0, None, 17, out.ctypes.data, None,
                                                    None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_render_adaptive_compute(None, None, None, 100, 0, None, 17, out.ctypes.data, None,
                                                     None) == L.MBK_ERR_INVALID
    assert (out == 0xA5).all()


def test_the_seahorse_centre_is_the_one_of_the_bla_tests():
    text = open(os.path.join(os.path.dirname(__file__), "test_gpu_deep_bla.py")).read()
    assert all(f'"{x}"' in text for x in K.SEAHORSE)


@pytest.mark.parametrize("name", list(K.CASES))
def test_the_middle_threshold_refines_some_pixels_and_leaves_others(name):
    _, view, _, _, mid = K.case(name)
    share = K.model_share(name, mid)
    print(name, view.width, view.height, "threshold", mid, "refined share", share)
    assert 0.05 <= share <= 0.60, share
    assert abs(share - SHARES[name]) < 0.0005, share          # the figure written beside the case
    if name in ("i-30", "i-30-two-tables", "i-200-two-tables"):
        c, _ = K.model_samples(name, 1)
        assert (c == 0).sum() == 1 and c[view.height // 2, view.width // 2] == 0     # c = i exactly: the one interior sample


def test_which_cases_need_two_tables():
    for name in K.TWO_TABLES:
        _, view, _, _, _ = K.case(name)
        for s in GPU_SUPERSAMPLES:
            assert B.dcmax(view) != B.dcmax(K.finer(view, s)), (name, s)
    _, view, _, _, _ = K.case("i-30")
    for s in GPU_SUPERSAMPLES:
        assert B.dcmax(view) == B.dcmax(K.finer(view, s)), s


def test_the_host_contract_does_not_care_what_kind_of_view_made_the_samples():
    name, s = "i-30", 2
    _, view, _, pal, mid = K.case(name)
    bc, bn = K.model_samples(name, 1)
    fc, fn = K.model_samples(name, s)
    for thr in (0, mid, 256):
        got, mask = render_adaptive_host(pal, s, thr, view.width, view.height, base_counts=bc, base_smooth=bn, fine_counts=fc,
                                         fine_smooth=fn, want_mask=True)
        want, want_mask = A.render_adaptive(pal.entries, pal.inside, pal.scale, pal.offset, s, thr, bc, bn, fc, fn)
        assert np.array_equal(got, want) and np.array_equal(mask, want_mask), thr
        if thr == mid:
            assert 0 < int(mask.sum()) < mask.size
