"""Relief shading on the host (include/mbk.h, "Relief shading"): mbk_normal_value_host, mbk_relief_shade_host and
mbk_relief_resolve_host -- compiled from the functions the kernels use -- held to the numpy model of the contract
(tests/relief_model.py) bit for bit, and the model itself held to the mathematics: the unit vector of z / (dz/dc) from the same
recurrences with mpmath, and the normals that are known in closed form on the real axis."""
import ctypes as C
import math

import numpy as np
import pytest

import distance_model as DM
import relief_model as RM
from distributedmandelbrot_amd import MbkError, Palette
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import normal_value_host, relief_shade_host
from distributedmandelbrot_amd.image import relief_resolve_host

# The truth runs at the 256 bits of distance_model's high-precision orbit plus 128.
TRUTH_BITS = DM.PRECISION_BITS + 128

# (c, the count, |model normal - true unit vector| (Euclidean) measured by test_model_against_mpmath at mrd 5000).  The bound a
# point is held to is twice its figure: the model is deterministic arithmetic without a libm call, so the figure can move only
# if the contract's operations do.  The error grows with the orbit's length and towards the boundary, where rounding in d is
# amplified exactly as in the distance estimate.
TRUTH_POINTS = [
    ((0.37, 0.6), 17, 1.448e-15),
    ((-0.1, 0.9), 23, 1.570e-15),
    ((-0.75, 0.1), 32, 3.077e-14),
    ((-1.75, 0.02), 12, 3.349e-14),
    ((-1.41, 0.001), 40, 3.223e-14),
    ((0.26, 0.001), 29, 3.642e-15),
    ((-0.7436438860371587, 0.1318259043091895), 1194, 6.031e-5),
]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _host_normals(zr, zi, dr, di, n):
    return np.array([normal_value_host(*(float(v) for v in s[:4]), int(s[4])) for s in zip(zr, zi, dr, di, n)], np.float64)


def _random_states(rng, count):
    """Final states as a kernel can hold them, and as it cannot: magnitudes over the whole exponent range."""
    e = rng.integers(-40, 70, size=(4, count)).astype(np.float64)
    v = rng.uniform(1.0, 2.0, size=(4, count)) * np.exp2(e) * rng.choice([-1.0, 1.0], size=(4, count))
    return v[0], v[1], v[2], v[3], rng.integers(1, 5000, size=count).astype(np.int32)


def test_normal_host_equals_the_model_on_random_states():
    rng = np.random.default_rng(20261020)
    zr, zi, dr, di, n = _random_states(rng, 3000)
    n[::17] = 0                                             # count 0: flat whatever the state
    # the states of real orbits: a view across the seahorse valley
    st = DM.states(*(a.ravel() for a in np.meshgrid(np.linspace(-0.8, -0.7, 24), np.linspace(0.05, 0.15, 24))), 400)
    zr, zi, dr, di = (np.concatenate([a, st[k]]) for a, k in ((zr, "zr"), (zi, "zi"), (dr, "dr"), (di, "di")))
    n = np.concatenate([n, st["n"]])
    got = _host_normals(zr, zi, dr, di, n)
    want = RM.normal(zr, zi, dr, di, n)
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.isnan(got).any()
    lit = (got != 0.0).any(axis=1)
    assert lit.sum() > 2800 and (~lit).sum() > 150
    assert np.abs(np.hypot(got[lit, 0], got[lit, 1]) - 1.0).max() <= 4 * np.finfo(np.float64).eps


def test_normal_host_special_states():
    inf, nan, sub, tiny = math.inf, math.nan, 5e-324, 2.0 ** -1040
    vals = [0.0, -0.0, 1.0, -1.5, sub, -sub, tiny, 1e-170, -1e-170, 1e-163, 1e-81, 1e78, -1e78, 1e155, 1e300, inf, -inf, nan]
    grid = np.array(np.meshgrid(vals, vals, vals, vals)).reshape(4, -1)
    zr, zi, dr, di = grid
    n = np.full(zr.size, 7, np.int32)
    got = _host_normals(zr, zi, dr, di, n)
    want = RM.normal(zr, zi, dr, di, n)
    assert np.array_equal(_bits(got), _bits(want))          # bit for bit: the sign of a zero component included
    assert not np.isnan(got).any()
    assert (np.signbit(got) & (got == 0.0)).any()           # ... and negative zeros do occur
    # a NaN or an infinity anywhere in w, |w| below 1e-162 (m underflows to 0) and |w| above 1e154 (m overflows): flat
    for state in [(nan, 1.0, 1.0, 1.0), (1.0, 1.0, inf, 1.0), (inf, 0.0, 0.0, 1.0), (1e-90, 1e-95, 1e-73, 1e-80),
                  (sub, sub, sub, sub), (0.0, -0.0, 1.0, 1.0), (1e78, 1e70, 1e77, 1e60), (1e155, 1.0, 1.0, 1.0),
                  (-1e100, 1e100, 1e100, 1e100)]:
        assert normal_value_host(*state, 3) == (0.0, 0.0), state
    with np.errstate(all="ignore"):
        w_small = abs(complex(1e-90, 1e-95) * complex(1e-73, -1e-80))
        w_large = abs(complex(1e78, 1e70) * complex(1e77, -1e60))
    assert 0.0 < w_small < 1e-162 and 1e154 < w_large < math.inf
    # inside the range (m a normal number) the normal is a unit vector
    for state in [(1e-75, 0.0, 1e-75, 0.0), (1e77, 0.0, 1e76, 0.0)]:
        assert normal_value_host(*state, 3) == (1.0, 0.0), state
    # count 0 (and a negative count, which no launch produces) is flat whatever the state
    assert normal_value_host(3.0, 4.0, 1.0, 2.0, 0) == (0.0, 0.0) and normal_value_host(3.0, 4.0, 1.0, 2.0, -1) == (0.0, 0.0)
    # by hand: z = 3 + 4i, d = 1: w = z, |w| = 5
    assert normal_value_host(3.0, 4.0, 1.0, 0.0, 1) == (0.6, 0.8)
    out = (C.c_double * 2)(7.0, 7.0)
    assert L.load().mbk_normal_value_host(1.0, 1.0, 1.0, 1.0, 1, None) == L.MBK_ERR_INVALID and tuple(out) == (7.0, 7.0)


def test_shade_host_equals_the_model():
    rng = np.random.default_rng(7)
    k = 4000
    ang = rng.uniform(0.0, 2.0 * np.pi, k)
    nx, ny = np.cos(ang), np.sin(ang)
    nx[::11], ny[::11] = 0.0, 0.0                          # flat normals
    nx[5::23], ny[5::23] = -0.0, -0.0
    la = rng.uniform(0.0, 2.0 * np.pi, k)
    lx, ly = np.cos(la), np.sin(la)
    lx[3::29], ly[3::29] = 1.0, -1.0                        # the corners of the range: g reaches sqrt(2)
    h = np.where(rng.random(k) < 0.2, 0.0, np.exp2(rng.uniform(-12.0, 10.0, k)))
    h[1::31] = 2.0 ** 10
    got = np.array([relief_shade_host(*(float(v) for v in s)) for s in zip(nx, ny, lx, ly, h)], np.int64)
    want = np.array([int(RM.shade(a, b, c, d, e)) for a, b, c, d, e in zip(nx, ny, lx, ly, h)], np.int64)
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 256 and len(np.unique(got)) > 200
    # by hand
    assert relief_shade_host(1.0, 0.0, 1.0, 0.0, 1.5) == 256          # facing the light: t = 1
    assert relief_shade_host(-1.0, 0.0, 1.0, 0.0, 1.5) == 51          # facing away: t = 0.5 / 2.5 = 0.2 (rounded up), floor(51.2)
    assert relief_shade_host(-1.0, 0.0, 1.0, 0.0, 0.5) == 0           # t < 0
    assert relief_shade_host(0.0, 0.0, 1.0, 0.0, 0.0) == 0            # flat at height 0: t = 0
    assert relief_shade_host(0.0, 0.0, 0.6, 0.8, 1.5) == 153          # the neutral brightness floor(256 * 0.6)
    assert relief_shade_host(0.0, 0.0, 0.0, 0.0, 2.0 ** 10) == 255    # floor(256 * 1024 / 1025)
    for hh in (0.0, 0.25, 1.0, 1.5, 3.0, 1000.0, 2.0 ** 10):
        assert relief_shade_host(0.0, 0.0, 0.3, -0.4, hh) == RM.neutral(hh) == math.floor(256.0 * (hh / (1.0 + hh)))


def test_model_against_mpmath():
    for (cr, ci), n_want, measured in TRUTH_POINTS:
        (nx, ny), n, extra = RM.point(cr, ci, 5000)
        assert n == n_want, (cr, ci, n)
        agrees, (tx, ty) = RM.hp_normal(cr, ci, n, extra, TRUTH_BITS)
        assert agrees, (cr, ci)
        err = math.hypot(nx - tx, ny - ty)
        print(f"c = {cr!r} + {ci!r}i: n {n}, run-on {extra}, normal ({nx!r}, {ny!r}), error {err:.3e} (bound {2 * measured:.3e})")
        assert err <= 2.0 * measured, (cr, ci, err)
        assert abs(math.hypot(nx, ny) - 1.0) <= 4 * np.finfo(np.float64).eps


def test_closed_forms():
    # real c > 1/4: z and d stay positive reals, w = z d > 0 and fl(sqrt(fl(w^2))) = w: exactly (1, +0)
    for c in (0.2500001, 0.26, 0.3, 0.5, 1.0, 1.9, 2.0, 3.5, 1e3, 1e30):
        (nx, ny), n, _ = RM.point(c, 0.0, 20000)
        assert n > 0 and (nx, ny) == (1.0, 0.0) and not math.copysign(1.0, ny) < 0, c
        assert normal_value_host(*_final_state(c, 0.0, 20000)) == (1.0, 0.0)
    # real c < -2: z_1 = c^2 + c > 2 and d_1 = 2 c + 1 < 0; z stays positive and d negative: nx = -1, ny a zero
    for c in (-2.0000001, -2.5, -3.0, -10.0, -1e30):
        (nx, ny), n, _ = RM.point(c, 0.0, 100)
        assert n == 1 and nx == -1.0 and ny == 0.0, c
    # c = -2: z_1 = 2 exactly (n = 1) and z stays there, so the run-on takes all its 64 steps while d = -(4^k) - ... stays finite
    (nx, ny), n, extra = RM.point(-2.0, 0.0, 100)
    assert n == 1 and extra == DM.RUN_ON and nx == -1.0 and ny == 0.0
    zr, zi, dr, di, _ = _final_state(-2.0, 0.0, 100)
    assert (zr, zi) == (2.0, 0.0) and math.isfinite(dr) and dr < -2.0 ** 128
    # |c| ~ 1e80: z_1 ~ 1e160 escapes with mag = inf, and |z conj(d)|^2 overflows: flat
    for c in ((1e80, 0.0), (-1e80, 0.0), (3e79, -1e80)):
        assert RM.point(*c, 100) == ((0.0, 0.0), 1, 0), c
    # the conjugate point has the conjugate normal, bit for bit
    cr, ci = np.meshgrid(np.linspace(-2.1, 0.6, 37), np.linspace(0.01, 1.2, 23))
    up = DM.states(cr.ravel(), ci.ravel(), 300)
    down = DM.states(cr.ravel(), -ci.ravel(), 300)
    a = RM.normal(up["zr"], up["zi"], up["dr"], up["di"], up["n"])
    b = RM.normal(down["zr"], down["zi"], down["dr"], down["di"], down["n"])
    assert np.array_equal(up["n"], down["n"]) and (up["n"] > 0).sum() > 400
    lit = up["n"] > 0
    assert np.array_equal(_bits(a[lit, 0]), _bits(b[lit, 0])) and np.array_equal(_bits(a[lit, 1]), _bits(-b[lit, 1]))
    # mrd 0 and 1 run no step: flat everywhere
    for mrd in (0, 1):
        assert RM.point(0.3, 0.5, mrd) == ((0.0, 0.0), 0, 0)


def _final_state(cr, ci, mrd):
    st = DM.states([cr], [ci], mrd)
    return tuple(float(st[k][0]) for k in ("zr", "zi", "dr", "di")) + (int(st["n"][0]),)


def _palette(n=37, scale=2.3, offset=0.4):
    rng = np.random.default_rng(n)
    return Palette(rng.integers(0, 256, size=(n, 4), dtype=np.uint8), inside=(9, 200, 31, 77), scale=scale, offset=offset)


def _samples(rng, hs, ws):
    counts = rng.integers(0, 60, size=(hs, ws)).astype(np.int32)
    counts[rng.random((hs, ws)) < 0.25] = 0
    nu = np.where(counts > 0, counts + rng.uniform(-1.0, 1.0, size=(hs, ws)), 0.0)
    ang = rng.uniform(0.0, 2.0 * np.pi, size=(hs, ws))
    nrm = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    nrm[rng.random((hs, ws)) < 0.2] = 0.0                  # flat normals among the escaped samples
    nrm[counts == 0] = 0.0
    return counts, nu, nrm


@pytest.mark.parametrize("s", RM.R.SUPERSAMPLES)
def test_resolve_host_equals_the_model(s):
    rng = np.random.default_rng(100 + s)
    w, h = 7, 5
    pal = _palette()
    counts, nu, nrm = _samples(rng, h * s, w * s)
    for light, height in (((math.cos(0.7), math.sin(0.7)), 1.5), ((-1.0, 1.0), 0.0), ((0.0, 0.0), 2.0 ** 10), ((0.3, -0.9), 0.125)):
        got = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=nrm, light=light, height=height)
        want = RM.render(pal.entries, pal.inside, pal.scale, pal.offset, light[0], light[1], height, s, counts, nu, nrm)
        assert np.array_equal(got, want), (s, light, height)
    # the default light is (cos, sin) of 45 degrees at height 1.5
    got = relief_resolve_host(pal, s, w, h, counts=counts, smooth=nu, normals=nrm)
    lx, ly = float(np.cos(np.deg2rad(45.0))), float(np.sin(np.deg2rad(45.0)))
    assert np.array_equal(got, RM.render(pal.entries, pal.inside, pal.scale, pal.offset, lx, ly, 1.5, s, counts, nu, nrm))


def test_resolve_host_colour_rules():
    rng = np.random.default_rng(5)
    pal = _palette()
    w, h = 9, 6
    counts, nu, _ = _samples(rng, h, w)
    esc = counts > 0
    assert esc.sum() > 20 and (~esc).sum() > 5
    smooth = RM.R.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, 1, counts, nu)
    flat = np.zeros((h, w, 2))
    # flat normals take the neutral q, whatever the light
    for height in (0.0, 0.5, 1.5, 2.0 ** 10):
        q = RM.neutral(height)
        got = relief_resolve_host(pal, 1, w, h, counts=counts, smooth=nu, normals=flat, light=(0.6, -0.8), height=height)
        want = smooth.astype(np.int64)
        want[..., :3] = (want[..., :3] * q + 128) >> 8
        want[~esc] = pal.inside
        assert np.array_equal(got, want), height
    # t >= 1: the smooth colour unchanged
    facing = np.broadcast_to(np.array([1.0, 0.0]), (h, w, 2))
    got = relief_resolve_host(pal, 1, w, h, counts=counts, smooth=nu, normals=facing, light=(1.0, 0.0), height=1.5)
    assert np.array_equal(got, smooth)
    # q = 0: black with the base's alpha; `inside` is not shaded
    got = relief_resolve_host(pal, 1, w, h, counts=counts, smooth=nu, normals=-facing, light=(1.0, 0.0), height=0.5)
    assert (got[esc][:, :3] == 0).all() and np.array_equal(got[esc][:, 3], smooth[esc][:, 3])
    assert (got[~esc] == np.array(pal.inside, np.uint8)).all()
    assert len(np.unique(smooth[esc][:, 3])) > 5                  # (the alphas of this palette do differ)


def test_host_refusals():
    lib = L.load()
    pal = _palette()
    w, h = 4, 3
    counts, nu, nrm = _samples(np.random.default_rng(1), h, w)
    out = np.full((h, w, 4), 0xAB, np.uint8)

    def call(spec, width=w, height=h, c=counts, v=nu, m=nrm, o=out):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return lib.mbk_relief_resolve_host(C.byref(spec) if spec is not None else None, width, height, ptr(c), ptr(v), ptr(m), ptr(o))

    assert call(pal.relief_spec(1)) == L.MBK_OK and not (out == 0xAB).all()
    out[:] = 0xAB
    bad = [pal.relief_spec(s) for s in (0, 5, 6, 7, 9, 16)]
    bad += [pal.relief_spec(1, light=l) for l in ((1.0000001, 0.0), (0.0, -1.5), (math.nan, 0.0), (0.0, math.inf), (-math.inf, 0.0))]
    bad += [pal.relief_spec(1, height=x) for x in (-1e-300, -1.0, 2.0 ** 10 + 1.0, math.nan, math.inf)]
    bad += [Palette(pal.entries[:1], scale=1.0).relief_spec(1)]
    bad += [Palette(pal.entries, scale=x).relief_spec(1) for x in (0.0, -1.0, 2.0 ** 21, math.nan)]
    bad += [Palette(pal.entries, offset=x).relief_spec(1) for x in (2.0 ** 21, math.nan)]
    no_palette = pal.relief_spec(1)
    no_palette.palette = None
    bad.append(no_palette)
    for spec in bad:
        assert call(spec) == L.MBK_ERR_INVALID
    assert call(None) == L.MBK_ERR_INVALID
    ok = pal.relief_spec(1)
    assert call(ok, c=None) == call(ok, v=None) == call(ok, m=None) == L.MBK_ERR_INVALID
    assert call(ok, width=0) == call(ok, height=0) == L.MBK_ERR_INVALID
    assert lib.mbk_relief_resolve_host(C.byref(ok), w, h, counts.ctypes.data, nu.ctypes.data, nrm.ctypes.data, None) == L.MBK_ERR_INVALID
    assert (out == 0xAB).all()                               # a refusal writes nothing
    # the edges of the ranges are inside them
    for spec in (pal.relief_spec(1, light=(1.0, -1.0)), pal.relief_spec(1, height=0.0), pal.relief_spec(1, height=2.0 ** 10)):
        assert call(spec) == L.MBK_OK
    with pytest.raises(MbkError):
        relief_resolve_host(pal, 1, w, h, counts=counts, smooth=nu, normals=nrm, height=-1.0)
    with pytest.raises(ValueError):
        relief_resolve_host(pal, 2, w, h, counts=counts, smooth=nu, normals=nrm)


def test_struct_layout():
    # uint32, pointer, uint32, uint8[4], five doubles, uint32 (+ tail padding): the header's field order
    assert C.sizeof(L.mbk_relief_spec) == 8 + 8 + 4 + 4 + 5 * 8 + 8
    assert L.mbk_relief_spec.light_x.offset == 40 and L.mbk_relief_spec.max_band_rows.offset == 64
