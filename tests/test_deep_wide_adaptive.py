"""CPU tests of adaptive supersampling of extended-range deep views (include/mbk.h, the section of that name): the new entry
points are declared, bind and refuse a NULL ctx, and the shared cases (tests/deep_wide_adaptive_cases.py) are what the GPU
tests need them to be -- middle thresholds that refine neither nothing nor everything, shapes whose base and fine views need
two wide bilinear-approximation tables and shapes whose views share one."""
import os
import re

import numpy as np
import pytest

import deep_wide_adaptive_cases as K
import deep_wide_bla_model as X
from distributedmandelbrot_amd import MandelbrotDevice
from distributedmandelbrot_amd import _lib as L

NEW_SYMBOLS = ["mbk_deep_xview_render_adaptive_launch", "mbk_deep_xview_render_adaptive_compute"]
GPU_SUPERSAMPLES = (2, 3, 4, 8)      # render_model.SUPERSAMPLES past 1, which has no finer view

# the refined share of the model's mask at the middle threshold on the library's wide table, W x H (the share test prints them)
SHARES = {"i-1100": 0.1506, "i-1100-two-tables": 0.1538, "i-3000-two-tables": 0.1562, "mis-1100": 0.2882, "short-1100": 0.1532,
          "1e-400": 0.2842}


def test_the_new_symbols_bind_and_refuse_a_null_ctx():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mbk_abi_version() == 5
    for name in ("render_wide_view_adaptive", "launch_render_wide_view_adaptive"):
        assert callable(getattr(MandelbrotDevice, name))
    out = np.full(16, 0xA5, np.uint8)
    assert lib.mbk_deep_xview_render_adaptive_launch(None, None, None, 100, 0, None, 17, out.ctypes.data, None,
                                                     None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_xview_render_adaptive_compute(None, None, None, 100, 0, None, 17, out.ctypes.data, None,
                                                      None) == L.MBK_ERR_INVALID
    assert (out == 0xA5).all()


def test_the_header_declares_the_new_symbols():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "mbk.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int " + name + r"\(mbk_ctx \*ctx, const mbk_deep_orbit \*orbit, const mbk_deep_xview \*view,", text, re.M), name


@pytest.mark.parametrize("name", list(K.CASES))
def test_the_middle_threshold_refines_some_pixels_and_leaves_others(name):
    _, view, _, _, mid = K.case(name)
    share = K.model_share(name, mid)
    print(name, view.width, view.height, "threshold", mid, "refined share", share)
    assert 0.05 <= share <= 0.60, share
    assert abs(share - SHARES[name]) < 0.0005, share          # the figure written beside the case


def test_which_cases_need_two_tables():
    assert set(K.TWO_TABLES) | set(K.ONE_TABLE) == set(K.CASES)
    for name in K.TWO_TABLES:
        _, view, _, _, _ = K.case(name)
        for s in GPU_SUPERSAMPLES:
            assert X.dcmax(view) != X.dcmax(K.finer(view, s)), (name, s)
    for name in K.ONE_TABLE:
        _, view, _, _, _ = K.case(name)
        for s in GPU_SUPERSAMPLES:
            assert X.dcmax(view) == X.dcmax(K.finer(view, s)), (name, s)
