"""Distance estimates for deep views on the CPU (include/mbk.h, "Distance estimates for deep views"): the numpy model of the
contract (tests/deep_distance_model.py, what the GPU is held to bit for bit) against the truth in mpmath, the need for and the
exactness of the scaled derivative, Koebe's bound, the output rule on the host, the colour rule of MBK_RENDER_DISTANCE_REL and
the palette helpers.  No GPU."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

import deep_distance_model as DD
import deep_model as D
import distance_model as M
import render_model as R
from distributedmandelbrot_amd import DeepOrbit, DeepView, MbkError, Palette
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import resolve_host
from test_deep_truth import M41, M51

# name -> (centre, span, mrd)
CASES = {
    "i-1e-30": (("0", "1"), 1e-30, 3000),
    "i-1e-200": (("0", "1"), 1e-200, 3000),
    "i-1e-280": (("0", "1"), 1e-280, 3000),
    "M51-1e-35": (M51, 1e-35, 3000),
    "M41-1e-25": (M41, 1e-25, 3000),
    "seahorse-1e-12": (("-0.77568377", "0.13646737"), 1e-12, 3000),
}
PICKS = 100
_CACHE = {}


def _case(name):
    """The seeded picks of a 64 x 64 view, as test_deep_truth._sample makes them, and the model's states on them."""
    if name not in _CACHE:
        centre, span, mrd = CASES[name]
        orbit = DeepOrbit(*centre, mrd, min_span=span)
        view = DeepView(span, 64, 64)
        dr, di = D.offsets(view)
        pick = np.random.RandomState(1).choice(dr.size, PICKS, replace=False)
        zr, zi = orbit.table()
        st = DD.states(zr, zi, dr[pick], di[pick], mrd)
        _CACHE[name] = (orbit, view, dr[pick], di[pick], st)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_model_against_truth(name):
    centre, span, mrd = CASES[name]
    orbit, view, dr, di, st = _case(name)
    rel = DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"])
    esc = np.flatnonzero(st["n"] > 0)
    assert len(np.unique(st["n"])) >= 8, np.unique(st["n"])
    assert esc.size >= 0.9 * PICKS, esc.size
    errs, agree = [], 0
    for i in esc:
        ok, truth = DD.hp_sample(centre, dr[i], di[i], span, st["n"][i], st["extra"][i], orbit.precision_bits + 128)
        if ok:
            agree += 1
            errs.append(abs(rel[i] - truth) / truth)
    worst = max(errs)
    print(f"{name}: {esc.size} of {PICKS} escaped, {agree} agree in (count, run-on), {len(np.unique(st['n']))} distinct counts "
          f"{st['n'][esc].min()}..{st['n'][esc].max()}, e up to {int(st['e'].max())}, worst relative error of rel {worst:.3e}")
    assert agree >= 0.99 * esc.size, (agree, esc.size)
    assert np.isfinite(rel[esc]).all() and (rel[esc] > 0).all()
    assert worst <= DD.DEEP_DERIVATIVE_REL, worst
    assert DD.DEEP_DERIVATIVE_REL <= 1e-4


def test_the_scaling_is_needed_and_exact():
    centre, span, mrd = CASES["i-1e-200"]
    orbit, view, dr, di, st = _case("i-1e-200")
    zr, zi = orbit.table()
    frozen = DD.states(zr, zi, dr, di, mrd, freeze_e=True)
    esc = st["n"] > 0
    assert esc.sum() >= 90 and np.array_equal(frozen["n"], st["n"]) and np.array_equal(frozen["extra"], st["extra"])
    assert not np.isfinite(frozen["dmagD"][esc]).any()          # the plain contract's "0" on every escaped pixel
    assert (st["e"][esc] >= 512).all() and (st["e"] % 256 == 0).all()
    rel = DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"])
    assert np.isfinite(rel[esc]).all() and (rel[esc] > 0).all()
    assert (st["dmagD"][esc] < 2.0 ** 513).all()
    # where nothing is rescaled the scaled model IS the plain binary64 derivative, bit for bit
    centre, span, mrd = CASES["i-1e-30"]
    orbit, view, dr, di, st = _case("i-1e-30")
    zr, zi = orbit.table()
    frozen = DD.states(zr, zi, dr, di, mrd, freeze_e=True)
    assert not st["e"].any()
    for k in ("n", "extra", "Dr", "Di", "mag", "dmagD"):
        assert np.array_equal(frozen[k], st[k]), k


def test_koebe_bound_at_1e_200():
    """The centre c = i is in the set, so the true distance of a pixel is at most |dc| and de <= 4 |dc|."""
    centre, span, mrd = CASES["i-1e-200"]
    orbit, view, dr, di, st = _case("i-1e-200")
    rel = DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"])
    esc = st["n"] > 0
    ratio = rel[esc] / (4.0 * (np.hypot(dr[esc], di[esc]) / span))      # (lengths as fractions of the span: no underflow)
    print(f"largest rel x span / (4 |dc|): {ratio.max():.4f}")
    assert (ratio <= 1.0 + DD.DEEP_DERIVATIVE_REL).all() and ratio.max() > 0.01


def _host(lib, mag, dmagD, e, range_r, n):
    return lib.mbk_deep_distance_value_host(float(mag), float(dmagD), int(e), float(range_r), int(n))


def test_output_rule_against_mpmath():
    lib = L.load()
    worst, at = 0.0, None
    for name, (centre, span, mrd) in CASES.items():
        st = _case(name)[4]
        f, k = math.frexp(span)
        want_model = DD.value(st["mag"], st["dmagD"], st["e"], span, st["n"])
        for i in range(PICKS):
            got = _host(lib, st["mag"][i], st["dmagD"][i], st["e"][i], span, st["n"][i])
            if st["n"][i] <= 0:
                assert got == 0.0
                continue
            assert got == want_model[i], (name, i)       # numpy's ln is glibc's: the model and the host agree to the bit
            near, v = DD.expression_true(st["mag"][i], st["dmagD"][i], span)
            g = math.ldexp(got, int(st["e"][i]) + k)      # exact: rel is a normal number on every case
            err = float(abs(mpmath.mpf(g) - v) / mpmath.mpf(float(np.spacing(near))))
            if err > worst:
                worst, at = err, (name, i, float(st["mag"][i]), float(st["dmagD"][i]), int(st["e"][i]))
    print(f"mbk_deep_distance_value_host: worst {worst:.4f} ulp against the correctly rounded expression at {at}")
    assert worst <= DD.DD0, (worst, at)
    assert DD.DD0 - worst <= 0.1, (worst, "DD0 is stale: set it to the measurement rounded up to two decimals")


def test_output_rule_special_values():
    lib = L.load()
    assert _host(lib, 1e10, 1e300, 512, 1e-200, 0) == 0.0
    assert _host(lib, 1e10, 1e300, 512, 1e-200, -3) == 0.0
    assert _host(lib, 1e10, 0.0, 512, 1e-200, 5) == math.inf
    assert _host(lib, 1e10, math.nan, 0, 1e-20, 5) == 0.0
    assert _host(lib, math.nan, 1e30, 0, 1e-20, 5) == 0.0
    assert _host(lib, math.inf, math.inf, 0, 1e-20, 5) == 0.0
    # the exponents add up exactly: the same mantissa at every (e, range_r) pair
    base = _host(lib, 1e10, 1e40, 0, 0.75, 7)
    assert base > 0
    for e, k in ((256, -700), (1024, 2), (2048, -959), (768, -768)):
        assert _host(lib, 1e10, 1e40, e, math.ldexp(0.75, k), 7) == math.ldexp(base, -(e + k)), (e, k)
    # a result below 2^-1022 rounds once: it is ldexp of a mantissa within 3 ulps (DD0 < 3) of the correctly rounded one
    near, _ = DD.expression_true(1e10, 1e40, 0.75)
    assert abs(base - near) <= 3 * np.spacing(near)
    for e in (980, 1000, 1020):
        got = _host(lib, 1e10, 1e40, e, 0.75, 7)
        assert 0.0 < got < 2.0 ** -1022
        cands, g = set(), near
        lo = near
        for _ in range(3):
            lo = np.nextafter(lo, 0.0)
        g = lo
        for _ in range(7):
            cands.add(math.ldexp(float(g), -e))
            g = np.nextafter(g, np.inf)
        assert got in cands and got == math.ldexp(base, -e), e
    assert _host(lib, 1e10, 1e40, 1 << 30, 0.75, 7) == 0.0


@pytest.mark.parametrize("s", [1, 2, 3, 4, 8])
def test_resolve_host_with_the_relative_source(s):
    assert L.RENDER_SOURCES["distance_rel"] == 4 == L.MBK_RENDER_DISTANCE_REL
    rs = np.random.RandomState(40 + s)
    w, h = 37, 23
    counts = rs.randint(0, 50, (h * s, w * s)).astype(np.int32)
    rel = np.exp(rs.uniform(-12, 1, counts.shape))
    rel[rs.rand(*counts.shape) < 0.02] = math.inf
    rel[counts == 0] = 0.0
    view = DeepView(1e-100, w, h)
    pal = Palette(rs.randint(0, 256, (200, 4)).astype(np.uint8), inside=(1, 2, 3, 255)).for_deep_distance(view, 9.0, inner_px=0.5)
    got = resolve_host(pal, "distance_rel", s, w, h, counts=counts, smooth=rel)
    want = R.resolve(M.colour_distance(pal.entries, pal.inside, pal.scale, pal.offset, counts, rel), s)
    assert np.array_equal(got, want)
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 50
    # the two distance sources share the colour rule
    assert np.array_equal(got, resolve_host(pal, "distance", s, w, h, counts=counts, smooth=rel))
    for bad in (Palette(pal.entries, scale=2.0 ** 81), Palette(pal.entries, scale=0.0), Palette(pal.entries[:1])):
        with pytest.raises(MbkError):
            resolve_host(bad, "distance_rel", s, w, h, counts=counts, smooth=rel)
    with pytest.raises(MbkError):
        resolve_host(pal, "distance_rel", s, w, h, counts=counts)


def test_palette_helpers():
    view = DeepView(1e-250, 801, 601)
    pal = Palette.deep_distance(view, 8.0, inner_px=1.0, n=256)
    assert len(pal) == 256 and tuple(pal.entries[0]) == (0, 0, 0, 255) and tuple(pal.entries[-1]) == (255, 255, 255, 255)
    assert pal.scale == 255 * 800 / 7.0 and pal.offset == -255 / 7.0
    # rel of one output pixel is 1 / (W - 1): entry 0 at inner_px, the last entry at width_px, whatever the span
    assert abs((1.0 / 800) * pal.scale + pal.offset) < 1e-9
    assert abs((8.0 / 800) * pal.scale + pal.offset - 255) < 1e-9
    other = Palette.deep_distance(DeepView(1e-20, 801, 601), 8.0, inner_px=1.0)
    assert (other.scale, other.offset) == (pal.scale, pal.offset)
    base = Palette(np.zeros((10, 4), np.uint8))
    assert base.for_deep_distance(view, 3.0).scale == 9 * 800 / 3.0 and base.for_deep_distance(view, 3.0).offset == 0.0
    with pytest.raises(ValueError):
        base.for_deep_distance(view, 1.0, inner_px=1.0)
    assert Palette.deep_distance(view).scale == 255 * 800 / 8.0
    # the plain helper is unchanged
    from distributedmandelbrot_amd import View
    assert Palette.distance(View(-2.0, -1.5, 3.0, 3.0, 301, 301), 8.0).scale == 255 / (8.0 * (3.0 / 300))


def test_signatures_and_symbols():
    lib = L.load()
    for name in ("mbk_deep_view_launch_distance", "mbk_deep_view_compute_distance", "mbk_deep_distance_value_host"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.mbk_abi_version() == 5
    assert lib.mbk_deep_view_launch_distance(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_deep_view_compute_distance(None, None, None, 10, 0, None, None, None) == L.MBK_ERR_INVALID
