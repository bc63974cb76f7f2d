"""CPU tests of the deep-zoom views' host side (include/mbk.h, "Deep-zoom views"): the decimal parser, the fixed-point
reference orbit, the numpy model of the step against direct high-precision iteration, and the ABI-5 bindings.  None of
them needs a GPU: an orbit needs no device and no ctx."""
import ctypes as C
import math
from decimal import Decimal
from fractions import Fraction

import numpy as np
import pytest

import deep_model as D

SEAHORSE = ("-0.743643887037158704752191506114774", "0.131825904205311970493132056385139")


def _lib():
    from distributedmandelbrot_amd import _lib as L
    return L, L.load()


def _create(cr, ci, bits=64, mrd=2):
    L, lib = _lib()
    h = C.c_void_p()
    st = lib.mbk_deep_orbit_create(cr.encode() if isinstance(cr, str) else cr, ci.encode() if isinstance(ci, str) else ci,
                                   bits, mrd, C.byref(h))
    if st == L.MBK_OK:
        lib.mbk_deep_orbit_destroy(h)
    return st


def test_abi_5_and_the_deep_symbols_bind():
    L, lib = _lib()
    assert L.MBK_ABI_VERSION == 5 and lib.mbk_abi_version() == 5
    for name in ("mbk_deep_orbit_create", "mbk_deep_orbit_destroy", "mbk_deep_orbit_info", "mbk_deep_orbit_read",
                 "mbk_deep_view_launch", "mbk_deep_view_compute", "mbk_deep_view_submit"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(L.mbk_deep_view) == 2 * 8 + 6 * 4
    import distributedmandelbrot_amd as m
    assert m.DeepOrbit and m.DeepView and "DeepOrbit" in m.__all__ and "DeepView" in m.__all__


ACCEPTED = ["0", "-0", "+1", "1.5", "-3.99999999", "1e-3", "1.25E+0", "0.1e1", "00012e-4", "3.9e0",
            "1" + "0" * 60 + "e-60", "-0.000000000000000000000000000000000001", "2E-400", "7e-5000"]


@pytest.mark.parametrize("s", ACCEPTED)
def test_parser_accepts_and_truncates_toward_zero(s):
    _check_parsed(s, 128)


@pytest.mark.parametrize("s", ACCEPTED)
def test_parser_accepts_and_truncates_toward_zero_at_4096_bits(s):
    _check_parsed(s, 4096)


def _check_parsed(s, P):
    from distributedmandelbrot_amd import DeepOrbit
    o = DeepOrbit(s, "0", 2, precision_bits=P)
    v = D.exact(s)
    x = (abs(v.numerator) << P) // v.denominator        # floor(|C| 2^P)
    want = (-x if v < 0 else x) / (1 << P)                # Python rounds int / int correctly
    zr, zi = o.table()
    assert zr[1] == want and zi[1] == 0.0


@pytest.mark.parametrize("s", ["", " 1", "1 ", "1.", ".5", "1e", "1e+", "--1", "+-1", "0x1", "1,5", "nan", "inf", "4", "-4",
                               "4.0", "40e-1", "1e1", "1_0", "١", "1.5.2", "e5", "1e5.0"])
def test_parser_rejects(s):
    L, _ = _lib()
    assert _create(s, "0") == L.MBK_ERR_INVALID
    assert _create("0", s) == L.MBK_ERR_INVALID


def test_precision_and_mrd_limits():
    L, _ = _lib()
    for bits in (64, 128, 4096):
        assert _create("0.25", "0.5", bits) == L.MBK_OK
    for bits in (0, 32, 65, 100, 4160, 8192):
        assert _create("0.25", "0.5", bits) == L.MBK_ERR_INVALID
    assert _create("0.25", "0.5", 64, 0) == L.MBK_ERR_INVALID and _create("0.25", "0.5", 64, 1) == L.MBK_ERR_INVALID
    assert _create(None, "0.5") == L.MBK_ERR_INVALID


@pytest.mark.parametrize("c, zs, length, escaped", [
    (("0", "1"), [(0, 0), (0, 1), (-1, 1), (0, -1), (-1, 1), (0, -1), (-1, 1)], 40, False),
    (("-1", "0"), [(0, 0), (-1, 0), (0, 0), (-1, 0), (0, 0)], 40, False),
    (("-2", "0"), [(0, 0), (-2, 0)], 1, True),        # |Z_1|^2 = 4: escapes at once
    (("0", "0"), [(0, 0)] * 8, 40, False),
    (("1", "0"), [(0, 0), (1, 0), (2, 0)], 2, True),
])
def test_exact_orbits(c, zs, length, escaped):
    from distributedmandelbrot_amd import DeepOrbit
    o = DeepOrbit(c[0], c[1], 40, precision_bits=256)
    zr, zi = o.table()
    assert (o.length, o.escaped, o.precision_bits, o.mrd) == (length, escaped, 256, 40)
    assert zr.size == length + 1
    n = min(len(zs), zr.size)
    assert list(zip(zr[:n], zi[:n])) == [(float(a), float(b)) for a, b in zs[:n]]


@pytest.mark.parametrize("P", [192, 1024])
def test_generic_centre_within_one_ulp_of_2p_bits(P):
    from distributedmandelbrot_amd import DeepOrbit
    o = DeepOrbit(*SEAHORSE, 5000, precision_bits=P)
    zr, zi = o.table()
    ref, _, _ = D.fixed_orbit(*SEAHORSE, 2 * P, 200)
    for k in range(1, 201):
        for got, want in ((zr[k], ref[k][0]), (zi[k], ref[k][1])):
            w = want / (1 << (2 * P))
            assert abs(got - w) <= np.spacing(abs(w)), (k, got, w)


@pytest.mark.parametrize("c, P", [(("0.5", "0"), 128), (("0.3", "0.6"), 256), (("-0.75", "0.1"), 192), (("1e-21", "1"), 192)])
def test_escaping_centre_length_matches_the_restatement(c, P):
    from distributedmandelbrot_amd import DeepOrbit
    o = DeepOrbit(c[0], c[1], 10000, precision_bits=P)
    zs, M, esc = D.fixed_orbit(c[0], c[1], P, 10000)
    assert (o.length, o.escaped) == (M, esc) and esc
    zr, zi = o.table()
    assert [(a, b) for a, b in zip(zr, zi)] == [(x / (1 << P), y / (1 << P)) for x, y in zs]


@pytest.mark.parametrize("P", [64, 1024, 2048, 4096])
def test_generic_centre_table_is_exact_at_p(P):
    """Every entry of a 400-step orbit equals the restatement's fixed-point Z_k, correctly rounded to binary64."""
    from distributedmandelbrot_amd import DeepOrbit
    o = DeepOrbit(*SEAHORSE, 400, precision_bits=P)
    zs, M, esc = D.fixed_orbit(*SEAHORSE, P, 400)
    assert (o.length, o.escaped) == (M, esc) == (400, False)
    zr, zi = o.table()
    assert [(a, b) for a, b in zip(zr, zi)] == [(x / (1 << P), y / (1 << P)) for x, y in zs]


def _pow2_decimal(num: int, k: int) -> str:
    """num / 2^k as an exact decimal string."""
    return "%de-%d" % (num * 5 ** k, k)


@pytest.mark.parametrize("s, want", [
    ("1e-320", None),
    ("2.4703282292062327e-320", None),
    (_pow2_decimal(1, 1075), 0.0),                                  # exactly half the least subnormal: ties to even, 0
    (_pow2_decimal((1 << 3021) + 1, 4096), 2.0 ** -1074),           # 2^-1075 + 2^-4096: the sticky bit rounds up
    (_pow2_decimal((1 << 53) - 1, 1075), 2.0 ** -1022),             # largest subnormal + half an ulp: up to the normal
    (_pow2_decimal((1 << 53) - 3, 1075), (2 ** 52 - 2) * 2.0 ** -1074),   # a tie below it goes down to the even one
    (_pow2_decimal(3, 1075), 2.0 ** -1073),                         # 1.5 ulp: ties to even, up
], ids=["1e-320", "2.47e-320", "tie-2^-1075", "tie+sticky", "max-sub+half", "tie-down", "tie-up"])
@pytest.mark.parametrize("sign", ["", "-"])
def test_subnormal_rounding_at_4096_bits(s, want, sign):
    """fx_to_double below 2^-1022 (reachable only with P > 1022): one rounding, to nearest on the subnormal grid, ties to
    even, every dropped bit in the sticky; Python's int / int is the correctly rounded reference."""
    from distributedmandelbrot_amd import DeepOrbit
    P = 4096
    zr, zi = DeepOrbit("0", sign + s, 2, precision_bits=P).table()
    v = D.exact(s)
    x = (v.numerator << P) // v.denominator
    if want is not None:
        assert x / (1 << P) == want
    ref = (-x if sign else x) / (1 << P)                  # a negative value that rounds to zero is -0.0
    assert zi[1] == ref and math.copysign(1.0, zi[1]) == math.copysign(1.0, ref)


def test_python_centre_types_and_default_precision():
    from distributedmandelbrot_amd import DeepOrbit
    from distributedmandelbrot_amd.device import default_precision_bits
    assert default_precision_bits(1e-20) == 192 and default_precision_bits(1e-60) == 320
    assert default_precision_bits(None) == 1024 and default_precision_bits(1.0) == 64
    a = DeepOrbit("0.1", "-0.25", 50, min_span=1e-20).table()
    for cr, ci in ((Decimal("0.1"), Decimal("-0.25")), (Fraction(1, 10), Fraction(-1, 4))):
        b = DeepOrbit(cr, ci, 50, min_span=1e-20).table()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    third = DeepOrbit(Fraction(1, 3), 0, 2, precision_bits=192).table()[0][1]
    assert third == ((1 << 192) // 3) / (1 << 192)
    assert DeepOrbit(0.1, 0, 2, precision_bits=128).table()[0][1] == 0.1     # a float is taken exactly
    assert DeepOrbit(-1, 0, 2).table()[0][1] == -1.0


@pytest.mark.parametrize("centre, span, mrd", [(SEAHORSE, 1e-20, 30000), (("0", "1"), 1e-60, 5000)])
def test_model_matches_direct_iteration(centre, span, mrd):
    """The numpy step (what the GPU is held to bit for bit) against z = z^2 + c iterated directly at P + 128 fraction bits,
    200 seeded pixels of a 64^2 view.  Measured when this test was written: 199 / 200 at 1e-20 (one pixel one step apart;
    also at P + 512 bits), 200 / 200 at 1e-60.  Threshold 99 %."""
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    o = DeepOrbit(*centre, mrd, min_span=span)
    zr, zi = o.table()
    dr, di = D.offsets(DeepView(span, 64))
    pick = np.random.RandomState(5).choice(dr.size, 200, replace=False)
    model, _ = D.model_counts(zr, zi, dr[pick], di[pick], mrd)
    direct = D.direct_counts(centre[0], centre[1], dr[pick], di[pick], mrd, o.precision_bits + 128)
    assert len(np.unique(direct)) >= 10
    assert (model == direct).mean() >= 0.99, (model != direct).sum()


def test_offsets_are_the_contract():
    from distributedmandelbrot_amd import DeepView
    v = DeepView(1e-20, 5, 3, 4e-21)
    dr, di = D.offsets(v)
    s = 1e-20 / 4
    assert list(dr[:5]) == [-2 * s, -1 * s, 0.0, s, 2 * s]
    assert list(di[::5]) == [-1 * (4e-21 / 2), 0.0, 4e-21 / 2]
    assert np.array_equal(D.offsets(DeepView(1e-9, 1))[0], [0.0])
    assert math.isclose(DeepView(1e-20, 65, 33).span_i, 5e-21)
