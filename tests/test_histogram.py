"""Count histograms and histogram-equalised colouring on the host (include/mbk.h, "Count histograms and histogram-equalised
colouring"): the host forms -- compiled from the functions the kernels use -- against the numpy restatement of the contract
(tests/histogram_model.py), bit for bit, and every refusal a host call can make."""
import ctypes as C

import numpy as np
import pytest

import histogram_model as H
from distributedmandelbrot_amd import MbkError, Palette
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import counts_histogram_host, equalize_lut, equalize_value, resolve_host

NEW_SYMBOLS = ["mbk_counts_histogram", "mbk_view_histogram_launch", "mbk_deep_view_histogram_launch",
               "mbk_view_histogram_compute", "mbk_deep_view_histogram_compute", "mbk_counts_histogram_host",
               "mbk_equalize_lut_host", "mbk_equalize_value_host", "mbk_view_render_equalized_launch",
               "mbk_view_render_equalized_compute", "mbk_deep_view_render_equalized_launch",
               "mbk_deep_view_render_equalized_compute", "mbk_render_resolve_equalized_host"]


def test_the_symbols_bind():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert L.MBK_RENDER_EQUALIZED == 5 and L.RENDER_SOURCES["equalized"] == 5
    assert L.MBK_HISTOGRAM_MAX_MRD == H.MAX_MRD == 1 << 20
    assert lib.mbk_abi_version() == 5


def test_host_histogram_equals_bincount():
    rs = np.random.RandomState(7)
    for mrd, n in [(1, 100), (2, 1000), (300, 50000), (30000, 200000), (H.MAX_MRD, 300000)]:
        counts = rs.randint(0, mrd, n).astype(np.int32)
        got = counts_histogram_host(counts, mrd)
        assert got.dtype == np.uint64 and got.shape == (mrd,)
        assert np.array_equal(got, H.histogram(counts, mrd)) and int(got.sum()) == n
    # all-equal counts, and accumulation into a table that is not empty
    got = counts_histogram_host(np.full(12345, 77, np.int32), 100)
    assert got[77] == 12345 and got.sum() == 12345
    again = counts_histogram_host(np.full(5, 3, np.int32), 100, got)
    assert again is got and got[77] == 12345 and got[3] == 5 and got.sum() == 12350
    assert counts_histogram_host(np.zeros(0, np.int32), 10).sum() == 0


def test_out_of_range_counts_are_skipped():
    rs = np.random.RandomState(8)
    mrd = 500
    counts = rs.randint(-50, 700, 100000).astype(np.int32)
    counts[:4] = [-(2 ** 31), 2 ** 31 - 1, mrd, -1]
    guard = np.full(mrd + 16, 0xA5A5A5A5A5A5A5A5, np.uint64)
    hist = guard[8:8 + mrd]
    hist[:] = 0
    counts_histogram_host(counts, mrd, hist)
    in_range = (counts >= 0) & (counts < mrd)
    assert 0 < in_range.sum() < counts.size
    assert np.array_equal(hist, H.histogram(counts, mrd)) and int(hist.sum()) == int(in_range.sum())
    assert (guard[:8] == 0xA5A5A5A5A5A5A5A5).all() and (guard[8 + mrd:] == 0xA5A5A5A5A5A5A5A5).all()


def _hists():
    rs = np.random.RandomState(9)
    out = {
        "mrd 1": np.array([5], np.uint64),
        "mrd 2, E = 0": np.array([9, 0], np.uint64),
        "mrd 2": np.array([9, 4], np.uint64),
        "E = 0": np.array([1000] + [0] * 99, np.uint64),
        "all zero": np.zeros(50, np.uint64),
        "single bin": np.bincount([37] * 11, minlength=64).astype(np.uint64),
        "single bin, the last": np.bincount([63] * 3, minlength=64).astype(np.uint64),
        "single bin, the first": np.bincount([1] * 3 + [0] * 9, minlength=64).astype(np.uint64),
        "random dense": rs.randint(0, 1000, 3000).astype(np.uint64),
        "random sparse": (rs.randint(0, 1000, 30000) * (rs.rand(30000) < 0.01)).astype(np.uint64),
        "thirds": np.array([0, 1, 1, 1], np.uint64),                 # quotients that are not binary fractions
        "large": np.array([0, 2 ** 51 - 1, 0, 0], np.uint64),        # 2 E = 2^52 - 2, just inside
    }
    return out


@pytest.mark.parametrize("name", list(_hists()))
def test_table_equals_the_model_bit_for_bit(name):
    hist = _hists()[name]
    mrd = hist.size
    got = equalize_lut(hist)
    want = H.lut(hist)
    assert got.shape == (mrd + 2,) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    assert np.array_equal(want.view(np.uint64), H.lut_fast(hist).view(np.uint64))
    # monotone, ends 0 and 1 (all zeros when nothing escaped)
    assert (np.diff(got) >= 0.0).all() and got[0] == 0.0 and got[1] == 0.0
    total = int(hist[1:].astype(object).sum()) if mrd > 1 else 0
    assert got[mrd + 1] == (1.0 if total else 0.0)
    if total == 0:
        assert (got == 0.0).all()


def test_table_at_the_largest_mrd():
    rs = np.random.RandomState(10)
    mrd = H.MAX_MRD
    hist = (rs.randint(0, 5000, mrd) * (rs.rand(mrd) < 0.3)).astype(np.uint64)
    got = equalize_lut(hist)
    assert np.array_equal(got.view(np.uint64), H.lut_fast(hist).view(np.uint64))
    assert (np.diff(got) >= 0.0).all() and got[0] == 0.0 and got[1] == 0.0 and got[mrd + 1] == 1.0
    head = hist[:2000].copy()
    assert np.array_equal(H.lut(head).view(np.uint64), H.lut_fast(head).view(np.uint64))


def test_table_refusals():
    lib = L.load()
    ok = np.array([0, 1, 2], np.uint64)
    lut = np.full(5 + 2, -7.0)
    out = lut[1:6]

    def call(h, mrd, dst=out):
        st = lib.mbk_equalize_lut_host(h.ctypes.data if h is not None else None, mrd, dst.ctypes.data if dst is not None else None)
        assert (lut == -7.0).all()
        return st

    assert call(None, 3) == L.MBK_ERR_INVALID
    assert call(ok, 3, None) == L.MBK_ERR_INVALID
    assert call(ok, 0) == L.MBK_ERR_INVALID
    assert call(np.zeros(8, np.uint64), H.MAX_MRD + 1) == L.MBK_ERR_INVALID
    # totals: numerator and denominator must stay below 2^53, so 2 E >= 2^53 is refused; count 0 takes no part
    assert call(np.array([0, 2 ** 52, 0], np.uint64), 3) == L.MBK_ERR_INVALID
    assert call(np.array([0, 2 ** 51, 2 ** 51], np.uint64), 3) == L.MBK_ERR_INVALID
    assert call(np.array([0, 2 ** 63, 2 ** 63], np.uint64), 3) == L.MBK_ERR_INVALID      # a sum that wraps 64 bits
    assert call(np.array([0, 2 ** 64 - 1, 1], np.uint64), 3) == L.MBK_ERR_INVALID
    inside = np.array([2 ** 60, 2 ** 51 - 1, 0], np.uint64)      # the largest total that passes; nothing outside mrd + 2 entries
    assert lib.mbk_equalize_lut_host(inside.ctypes.data, 3, out.ctypes.data) == L.MBK_OK
    assert (out == H.lut(inside)).all() and lut[0] == -7.0 and lut[6] == -7.0
    with pytest.raises(MbkError):
        equalize_lut(np.array([0, 2 ** 52], np.uint64))


def test_value_rule():
    rs = np.random.RandomState(11)
    for mrd in (1, 2, 7, 1000):
        hist = rs.randint(0, 100, mrd).astype(np.uint64)
        table = H.lut(hist)
        nus = [np.nan, -np.inf, -1.0, -0.0, 0.0, 0.5, 1.0, 1.25, mrd - 1.0, float(mrd), mrd + 0.5, mrd + 1.0, mrd + 1.5, 1e300,
               np.inf, np.nextafter(mrd + 1.0, 0.0), np.nextafter(1.0, 2.0)]
        nus += [float(k) for k in range(0, min(mrd + 2, 12))]
        nus += list(rs.uniform(0.0, mrd + 2.0, 2000))
        want = H.value(table, np.array(nus))
        got = np.array([equalize_value(table, nu) for nu in nus])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), mrd
        assert equalize_value(table, mrd + 1.0) == table[mrd + 1] and equalize_value(table, 1e300) == table[mrd + 1]
        assert equalize_value(table, np.nan) == 0.0 and equalize_value(table, -np.inf) == 0.0 and equalize_value(table, -1.0) == 0.0
        for k in range(0, mrd + 2):
            assert equalize_value(table, float(k)) == table[k]
    assert L.load().mbk_equalize_value_host(None, 5, 1.0) == 0.0


EQ_PAL = Palette(np.random.RandomState(12).randint(0, 256, (300, 4)).astype(np.uint8), inside=(9, 8, 7, 6)).for_equalized()


def _samples(rs, h, w, mrd):
    counts = rs.randint(0, mrd, (h, w)).astype(np.int32)
    counts[rs.rand(h, w) < 0.2] = 0
    nu = counts + rs.uniform(0.16, 1.53, (h, w))
    nu[counts == 0] = 0.0
    flat = nu.ravel()
    flat[:6] = [np.nan, -np.inf, -3.0, mrd + 1.0, 1e300, mrd + 0.5]
    counts.ravel()[:6] = 1
    return counts, nu


@pytest.mark.parametrize("s", [1, 2, 3])
def test_host_resolve_equals_the_model(s):
    rs = np.random.RandomState(13 + s)
    mrd, w, h = 400, 37, 29
    counts, nu = _samples(rs, h * s, w * s, mrd)
    table = H.lut(H.histogram(counts, mrd))
    for pal in (EQ_PAL, Palette(EQ_PAL.entries[:2], (1, 2, 3, 4), 0.7, 0.1), Palette(EQ_PAL.entries, (0, 0, 0, 255), 1000.0, -3.0)):
        got = resolve_host(pal, "equalized", s, w, h, counts=counts, smooth=nu, lut=table)
        want = H.render_equalized(pal.entries, pal.inside, pal.scale, pal.offset, table, s, counts, nu)
        assert np.array_equal(got, want), int((got != want).any(axis=2).sum())
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 20
    assert EQ_PAL.scale == len(EQ_PAL) - 1 and EQ_PAL.offset == 0.0


def test_resolve_refusals():
    lib = L.load()
    rs = np.random.RandomState(14)
    mrd, w, h = 50, 8, 6
    counts, nu = _samples(rs, h, w, mrd)
    table = H.lut(H.histogram(counts, mrd))
    pal = np.zeros((4, 4), np.uint8)
    out = np.full((h, w, 4), 0xA5, np.uint8)

    def spec(source=L.MBK_RENDER_EQUALIZED, s=1, n=4, scale=3.0, offset=0.0, palette=pal):
        return L.mbk_render_spec(source, s, palette.ctypes.data if palette is not None else None, n, (C.c_uint8 * 4)(0, 0, 0, 255),
                                 scale, offset, 0)

    def eq(sp, lut=table, lut_len=None, c=counts, v=nu, dst=out, width=w, height=h):
        st = lib.mbk_render_resolve_equalized_host(C.byref(sp) if sp is not None else None, lut.ctypes.data if lut is not None else None,
                                                   (lut.size if lut is not None else 0) if lut_len is None else lut_len, width, height,
                                                   c.ctypes.data if c is not None else None, v.ctypes.data if v is not None else None,
                                                   dst.ctypes.data if dst is not None else None)
        assert (out == 0xA5).all()
        return st

    def bad(k, x):
        t = table.copy()
        t[k] = x
        return t

    cases = {
        "NULL spec": lambda: eq(None), "NULL palette": lambda: eq(spec(palette=None)), "NULL table": lambda: eq(spec(), lut=None, lut_len=mrd + 2),
        "NULL counts": lambda: eq(spec(), c=None), "NULL nu": lambda: eq(spec(), v=None), "NULL output": lambda: eq(spec(), dst=None),
        "lut_len 0": lambda: eq(spec(), lut_len=0), "lut_len 1": lambda: eq(spec(), lut_len=1),
        "lut_len above the limit": lambda: eq(spec(), lut=np.zeros(H.MAX_MRD + 3), lut_len=H.MAX_MRD + 3),
        "entry > 1": lambda: eq(spec(), lut=bad(7, 1.0000001)), "entry < 0": lambda: eq(spec(), lut=bad(0, -1e-300)),
        "entry nan": lambda: eq(spec(), lut=bad(mrd + 1, np.nan)), "entry inf": lambda: eq(spec(), lut=bad(3, np.inf)),
        "source smooth": lambda: eq(spec(source=L.MBK_RENDER_SMOOTH)), "source bytes": lambda: eq(spec(source=L.MBK_RENDER_BYTES, n=256, palette=np.zeros((256, 4), np.uint8))),
        "source distance": lambda: eq(spec(source=L.MBK_RENDER_DISTANCE)), "source 6": lambda: eq(spec(source=6)),
        "palette of 1": lambda: eq(spec(n=1)), "palette of 65537": lambda: eq(spec(n=65537, palette=np.zeros((65537, 4), np.uint8))),
        "s = 5": lambda: eq(spec(s=5)), "scale 0": lambda: eq(spec(scale=0.0)), "scale > 2^20": lambda: eq(spec(scale=2.0 ** 21)),
        "scale nan": lambda: eq(spec(scale=np.nan)), "offset > 2^20": lambda: eq(spec(offset=2.0 ** 21)), "offset nan": lambda: eq(spec(offset=np.nan)),
        "width 0": lambda: eq(spec(), width=0), "height 0": lambda: eq(spec(), height=0),
    }
    for name, call in cases.items():
        assert call() == L.MBK_ERR_INVALID, name
    # the existing host resolve has no table: it still refuses the source
    st = lib.mbk_render_resolve_host(C.byref(spec()), w, h, counts.ctypes.data, None, nu.ctypes.data, out.ctypes.data)
    assert st == L.MBK_ERR_INVALID and (out == 0xA5).all()
    with pytest.raises(MbkError):
        resolve_host(EQ_PAL, "equalized", 1, w, h, counts=counts, smooth=nu)
    # and a call that is in order goes through
    ok = np.empty((h, w, 4), np.uint8)
    assert lib.mbk_render_resolve_equalized_host(C.byref(spec()), table.ctypes.data, table.size, w, h, counts.ctypes.data,
                                                 nu.ctypes.data, ok.ctypes.data) == L.MBK_OK


def test_histogram_host_refusals():
    lib = L.load()
    counts = np.arange(10, dtype=np.int32)
    hist = np.full(12, 3, np.uint64)
    assert lib.mbk_counts_histogram_host(None, 10, 10, hist.ctypes.data) == L.MBK_ERR_INVALID
    assert lib.mbk_counts_histogram_host(counts.ctypes.data, 10, 10, None) == L.MBK_ERR_INVALID
    assert lib.mbk_counts_histogram_host(counts.ctypes.data, 10, 0, hist.ctypes.data) == L.MBK_ERR_INVALID
    assert lib.mbk_counts_histogram_host(counts.ctypes.data, 10, H.MAX_MRD + 1, hist.ctypes.data) == L.MBK_ERR_INVALID
    assert (hist == 3).all()
    assert lib.mbk_counts_histogram_host(None, 0, 10, hist.ctypes.data) == L.MBK_OK and (hist == 3).all()
    with pytest.raises(MbkError):
        counts_histogram_host(counts, H.MAX_MRD + 1, np.zeros(H.MAX_MRD + 1, np.uint64))
