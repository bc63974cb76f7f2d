"""CPU tests of Julia views (include/mbk.h, "Julia views"): mbk_julia_count_host -- the contract's loop as the kernels restate
it, with the doubling a launch with that parameter would use -- against the literal numpy model of tests/julia_model.py, for
the count and the bits of mag; the identity with the Mandelbrot count; and the proof that the hazard the doubling rule guards
against is real (a guard test on cases where both forms agree would show nothing)."""
import ctypes as C

import numpy as np
import pytest

import julia_model as J

NAMED = [(-1.0, 0.0), (-0.75, 0.0), (0.25, 0.0), (0.0, 1.0), (-0.8, 0.156), (0.0, 0.0)]
OUTSIDE = [(1.5, 1.5)]
RING = [(-2.0, 0.0), (-2.0 + 1e-10, 0.0), (-2.0 - 1e-10, 0.0)]
PARAMS = NAMED + OUTSIDE + RING
MRDS = [0, 1, 2, 3, 1000]

# the hazard rows: c_i below, at and above the guard; z0_i subnormal or nearly so; |z0_r| in [0.3, 1.5].  The real parameters
# -1.8, -1.5 and -1.9 are chaotic on the real axis: a tiny zi grows by |2 zr| per step and the orbit escapes after some
# thousand steps, at a step that depends on the first, subnormal, products -- where the two forms of the doubling differ.
HAZARD_CI = [0.0, 1e-310, 2.0 ** -901, 2.0 ** -900]
HAZARD_CR = [-1.8, -1.5, -1.9, -0.75, -1.0]
HAZARD_Z0I = [5e-324, 1.5e-323, 1e-320, 1e-310, 1e-305, 1e-300]
HAZARD_Z0R = [0.3, 0.5, 0.7, 0.9, 1.1, 1.3, 1.5, -0.4, -0.8, -1.2]
HAZARD_MRD = 3000


def _lib():
    from distributedmandelbrot_amd import _lib as L
    return L, L.load()


def host_counts(z0r, z0i, c, mrd):
    """mbk_julia_count_host over the broadcast (z0r, z0i): (n int32, mag float64)."""
    L, lib = _lib()
    zr, zi = np.broadcast_arrays(np.asarray(z0r, np.float64), np.asarray(z0i, np.float64))
    n = np.zeros(zr.shape, np.int32)
    mag = np.zeros(zr.shape, np.float64)
    cn, cm = C.c_int32(0), C.c_double(0.0)
    for i in np.ndindex(zr.shape):
        assert lib.mbk_julia_count_host(float(zr[i]), float(zi[i]), float(c[0]), float(c[1]), int(mrd), C.byref(cn), C.byref(cm)) == L.MBK_OK
        n[i], mag[i] = cn.value, cm.value
    return n, mag


def same_bits(a, b):
    """Bitwise equality of two float64 arrays, any NaN equal to any NaN (IEEE leaves the payload of inf - inf open)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()


def assert_host_is_model(z0r, z0i, c, mrd, what):
    n, mag = host_counts(z0r, z0i, c, mrd)
    wn, wmag = J.julia_counts(z0r, z0i, c[0], c[1], mrd)
    assert np.array_equal(n, wn), (what, c, mrd, int((n != wn).sum()))
    assert same_bits(mag, wmag), (what, c, mrd)
    return n


def test_host_count_equals_the_model_on_random_pairs():
    rs = np.random.RandomState(11)
    total = 0
    for mrd in MRDS:
        k = 300 if mrd == 1000 else 100
        r, phi = 2.5 * np.sqrt(rs.uniform(size=(2, k))), rs.uniform(0, 2 * np.pi, size=(2, k))
        z, c = r[0] * np.exp(1j * phi[0]), r[1] * np.exp(1j * phi[1])
        for i in range(k):
            assert_host_is_model(z[i].real, z[i].imag, (c[i].real, c[i].imag), mrd, "random")
        total += k
    assert total >= 700


@pytest.mark.parametrize("c", PARAMS)
def test_host_count_equals_the_model_on_the_parameter_list(c):
    rs = np.random.RandomState(5)
    seen = set()
    for mrd in MRDS:
        z0r = np.concatenate([rs.uniform(-2.2, 2.2, 120), [c[0], 0.0, -c[0]]])
        z0i = np.concatenate([rs.uniform(-2.2, 2.2, 120), [c[1], 0.0, -c[1]]])
        seen.update(np.unique(assert_host_is_model(z0r, z0i, c, mrd, "list")).tolist())
    assert len(seen) > 3, seen


def test_host_count_equals_the_model_on_overflowing_and_nan_coordinates():
    big = [1e200, -1e200, 1e308, -1e308, 1e154, 1.3407807929942597e154, np.inf, np.nan]
    small = [0.0, 0.5, -1.0]
    for c in [(-1.0, 0.0), (-0.8, 0.156), (1.5, 1.5)]:
        for mrd in MRDS:
            for zr in big:
                assert_host_is_model(np.float64(zr), np.array(small + big), c, mrd, "odd")
                assert_host_is_model(np.array(small), np.float64(zr), c, mrd, "odd")


def test_host_count_equals_the_literal_model_on_the_hazard_rows_and_the_hazard_is_real():
    z0r = np.array(HAZARD_Z0R)[None, :]
    z0i = np.concatenate([HAZARD_Z0I, [-v for v in HAZARD_Z0I]])[:, None]
    differ = {}
    for cr in HAZARD_CR:
        for ci in HAZARD_CI:
            n = assert_host_is_model(z0r, z0i, (cr, ci), HAZARD_MRD, "hazard")
            fn, fmag = J.julia_counts(z0r, z0i, cr, ci, HAZARD_MRD, fma=True)
            ln, lmag = J.julia_counts(z0r, z0i, cr, ci, HAZARD_MRD)
            differ[(cr, ci)] = (int((fn != ln).sum()), int((fmag.view(np.uint64) != lmag.view(np.uint64)).sum()))
            assert np.array_equal(n, ln)
    # the rewrite fma(2, fl(zr zi), c_i) WOULD change counts below the guard ...
    assert differ[(-1.8, 0.0)][0] > 0 and differ[(-1.9, 0.0)][0] > 0 and differ[(-0.75, 0.0)][0] > 0, differ
    assert differ[(-1.8, 1e-310)][1] > 0, differ
    # ... and changes nothing at or above it: |c_i| >= 2^-900 swallows both candidate addends (2^-901 is refused all the same:
    # the rule is a bound, not the edge of the hazard)
    for cr in HAZARD_CR:
        assert differ[(cr, 2.0 ** -900)] == (0, 0), differ
    # one pinned case, so that the cases above cannot quietly lose their teeth: c = -1.8, z0 = (0.7, 5e-324)
    ln, _ = J.julia_counts(0.7, 5e-324, -1.8, 0.0, HAZARD_MRD)
    fn, _ = J.julia_counts(0.7, 5e-324, -1.8, 0.0, HAZARD_MRD, fma=True)
    hn, _ = host_counts(0.7, 5e-324, (-1.8, 0.0), HAZARD_MRD)
    assert int(ln) != int(fn) and int(hn) == int(ln) and int(ln) > 0, (int(ln), int(fn), int(hn))


def test_identity_with_the_mandelbrot_count(oracle, golden):
    from distributedmandelbrot_amd.device import julia_count_host
    pts = [(float(cr), float(ci), int(mrd)) for cr, ci, mrd in golden["points/inputs"]]
    assert len(pts) == 18
    for (cr, ci, mrd), ref in zip(pts, golden["points/counts"]):
        assert julia_count_host((cr, ci), (cr, ci), mrd)[0] == int(ref) == oracle.escape(cr, ci, mrd), (cr, ci, mrd)
    rs = np.random.RandomState(2)
    seen = set()
    for k in range(400):
        r, phi = 2.1 * np.sqrt(rs.uniform()), rs.uniform(0, 2 * np.pi)
        cr, ci = r * np.cos(phi), r * np.sin(phi)
        if k % 8 == 0:
            ci = 0.0          # the real axis: the literal loop
        mrd = int(rs.choice([2, 3, 50, 700]))
        n = julia_count_host((cr, ci), (cr, ci), mrd)[0]
        assert n == oracle.escape(cr, ci, mrd), (cr, ci, mrd)
        seen.add(n)
    assert 0 in seen and len(seen) > 8


def test_host_count_refusals_and_the_python_wrapper():
    L, lib = _lib()
    from distributedmandelbrot_amd.device import MbkError, julia_count_host
    n, mag = C.c_int32(77), C.c_double(7.5)
    for args in [(0.0, 0.0, np.nan, 0.0, 10), (0.0, 0.0, 0.0, np.inf, 10), (0.0, 0.0, 0.0, 0.0, 1 << 31)]:
        assert lib.mbk_julia_count_host(*args, C.byref(n), C.byref(mag)) == L.MBK_ERR_INVALID
        assert (n.value, mag.value) == (77, 7.5)
    assert lib.mbk_julia_count_host(0.0, 0.0, 0.0, 0.0, 10, None, C.byref(mag)) == L.MBK_ERR_INVALID
    assert lib.mbk_julia_count_host(2.0, 0.0, 0.0, 0.0, 10, C.byref(n), None) == L.MBK_OK and n.value == 1
    assert julia_count_host((2.0, 0.0), (0.0, 0.0), 10) == (1, 16.0)
    assert julia_count_host((2.0, 0.0), (0.0, 0.0), 1) == (0, 0.0)
    with pytest.raises(MbkError):
        julia_count_host((0.0, 0.0), (np.nan, 0.0), 10)


def test_the_model_quantiser_is_the_oracles(oracle):
    for mrd in (1, 2, 255, 256, 257, 1000, 4000):
        for c in {0, 1, 2, mrd // 2, mrd - 1}:
            if 0 <= c < mrd:
                assert int(J.quantise(c, mrd)) == oracle.quantise(c, mrd), (c, mrd)
