"""Stripe-average colouring on the host (include/mbk.h, "Stripe-average colouring"): mbk_stripe_state_host,
mbk_stripe_value_host, mbk_stripe_shade_host and mbk_stripe_resolve_host -- compiled from the functions the kernel uses -- held
to the numpy model of the contract (tests/stripe_model.py), the states bit for bit, and the model itself held to the
mathematics: the same recurrences with the true sin(s arg z_k) in mpmath, the cases that are known exactly, and continuity
across the escape bands."""
import ctypes as C
import math

import numpy as np
import pytest

import distance_model as DM
import stripe_model as SM
from distributedmandelbrot_amd import MbkError, Palette
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import stripe_shade_host, stripe_state_host, stripe_value_host
from distributedmandelbrot_amd.image import resolve_host, stripe_resolve_host

SEAHORSE = ((-0.765, 0.085, 0.04, 0.04 * 44 / 66, 67, 45), 600)      # the view of tests/test_gpu_relief.py
_HOST = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(h, m):
    """Two states of one pixel: the exact state on every bit; v to within the logarithms of two libraries (numpy's may be its
    own vector code, not the C library's)."""
    exact = all(h[k] == m[k] or (h[k] != h[k] and m[k] != m[k]) for k in ("n", "N", "cnt", "S", "t_last", "mag"))
    return exact and abs(h["v"] - m["v"]) <= 4.0 * np.spacing(abs(m["v"]))


def _host_view(v, mrd, density, skip):
    """The host twin on every pixel of a view tuple: dict of arrays [nrows, ncols], the value "v" among them."""
    key = (v, mrd, density, skip)
    if key not in _HOST:
        cr, ci = DM.axes(v)
        px = [stripe_state_host((x, y), mrd, density=density, skip=skip) for y in ci for x in cr]
        shape = (ci.size, cr.size)
        _HOST[key] = {k: np.array([p[k] for p in px], np.int32 if k in ("n", "N", "cnt") else np.float64).reshape(shape)
                      for k in ("n", "N", "cnt", "S", "t_last", "mag", "v")}
    return _HOST[key]


@pytest.mark.parametrize("skip", [0, 3])
@pytest.mark.parametrize("density", [1, 2, 5, 16])
def test_host_states_equal_the_model_on_every_bit(density, skip):
    v, mrd = SEAHORSE
    st, counts, mv = SM.model(v, mrd, density, skip)
    host = _host_view(v, mrd, density, skip)
    assert (counts == 0).sum() > 50 and len(np.unique(counts)) > 40
    for k in ("n", "N", "cnt"):
        assert np.array_equal(host[k], st[k]), k
    for k in ("S", "t_last", "mag"):
        assert np.array_equal(_bits(host[k]), _bits(st[k])), (k, int((_bits(host[k]) != _bits(st[k])).sum()))
    esc = counts > 0
    assert (st["N"][esc] > st["n"][esc]).all() and (st["N"][esc] - st["n"][esc] <= SM.RUN_ON).all()
    assert (st["cnt"][esc] == st["N"][esc] - skip).all() and (st["mag"][esc] >= SM.RADIUS2).all()
    assert not np.isnan(host["v"]).any() and not host["v"][~esc].any() and not st["S"][~esc].any()
    assert (host["v"][esc] > 0.0).all() and (host["v"][esc] < 1.0).all() and host["v"][esc].std() > 0.01
    # the value of the twin is the value function at the twin's state
    flat = {k: a.ravel() for k, a in host.items()}
    again = [stripe_value_host(*(t.item() for t in s)) for s in zip(flat["S"], flat["t_last"], flat["cnt"], flat["mag"], flat["n"])]
    assert np.array_equal(_bits(np.array(again)), _bits(flat["v"]))


def test_exact_cases():
    # c = 1 and c = -3: every counted point is real and positive: u = (1, 0) exactly, every t_k and v exactly 0.5 for any s
    for c, N in ((1.0, 5), (-3.0, 4)):
        for s in (1, 2, 5, 16):
            for skip in (0, 2):
                h = stripe_state_host((c, 0.0), 100, density=s, skip=skip)
                m = SM.point(c, 0.0, 100, s, skip)
                assert _same(h, m), (c, s, skip, h, m)
                assert h["n"] == 1 and h["N"] == N and h["cnt"] == N - skip and h["t_last"] == 0.5 and h["v"] == 0.5
                assert h["S"] == 0.5 * (N - skip)
    # c = -2: n = 1, z stays at 2, the run-on hits its 64-step cap, d = 1 - log2(ln 4 / (32 ln 2)) = 5 clamps to 1
    for s in (1, 5, 16):
        h = stripe_state_host((-2.0, 0.0), 100, density=s)
        assert _same(h, SM.point(-2.0, 0.0, 100, s))
        assert h["n"] == 1 and h["N"] == 1 + SM.RUN_ON == h["cnt"] and h["mag"] == 4.0 and h["S"] == 32.5 and h["v"] == 0.5
    assert stripe_value_host(10.0, 0.25, 20, 4.0, 1) == 0.5                      # d = 1: a1 itself
    assert stripe_value_host(10.0, 0.5, 20, 2.0 ** 64, 1) == 0.5                 # d = 0: a0 = 9.5 / 19
    assert stripe_value_host(10.0, 0.25, 20, 2.0 ** 65, 1) == (10.0 - 0.25) / 19.0      # d < 0 clamps to 0
    # c = 1e200: z_1 overflows, mag = inf, the term is 0.5, and no NaN appears
    for s in (1, 5, 16):
        h = stripe_state_host((1e200, 0.0), 100, density=s)
        assert _same(h, SM.point(1e200, 0.0, 100, s))
        assert (h["n"], h["N"], h["cnt"], h["S"], h["t_last"], h["v"]) == (1, 1, 1, 0.5, 0.5, 0.5) and h["mag"] == math.inf
    for state in ((3.0, 0.5, 4, math.inf, 1), (3.0, 0.5, 4, math.nan, 1), (3.0, 0.5, 4, 0.0, 1), (3.0, 0.5, 4, -1.0, 1)):
        v = stripe_value_host(*state)
        assert v == float(SM.value(*[np.array([x]) for x in state])[0]) and not math.isnan(v)
        assert v == (3.0 - 0.5) / 3.0                                            # d = 0 for a NaN: a0
    # skip >= N gives 0.5; skip = N - 1 gives S, the last term
    c = (0.37, 0.6)
    full = stripe_state_host(c, 5000, density=5)
    assert (full["n"], full["N"]) == (17, 21)
    for skip in (21, 22, 1000, 2 ** 31 - 1):
        h = stripe_state_host(c, 5000, density=5, skip=skip)
        assert _same(h, SM.point(*c, 5000, 5, skip)) and (h["cnt"], h["S"], h["t_last"], h["v"]) == (0, 0.0, 0.0, 0.5)
    h = stripe_state_host(c, 5000, density=5, skip=20)
    assert _same(h, SM.point(*c, 5000, 5, 20)) and h["cnt"] == 1 and h["S"] == h["t_last"] == full["t_last"] == h["v"]
    # mrd 0 and 1 run no step; mrd 2 runs one
    for mrd in (0, 1):
        h = stripe_state_host((0.37, 0.6), mrd, density=5)
        assert _same(h, SM.point(0.37, 0.6, mrd, 5)) and not any(h.values())
    h = stripe_state_host((1.5, 1.5), 2, density=5)
    assert _same(h, SM.point(1.5, 1.5, 2, 5)) and h["n"] == 1 and h["v"] > 0.0
    assert stripe_state_host((0.37, 0.6), 2, density=5)["n"] == 0
    # a count that is not positive stores 0 whatever the state
    assert stripe_value_host(3.0, 0.5, 4, 1e10, 0) == 0.0 and stripe_value_host(3.0, 0.5, 4, 1e10, -1) == 0.0


def test_value_against_the_correctly_rounded_value():
    v, mrd = SEAHORSE
    worst = 0.0
    for density, skip in ((1, 0), (5, 3), (16, 0)):
        host = _host_view(v, mrd, density, skip)
        e = SM.value_err_ulps(host["v"], host)
        assert not np.isnan(e).any()
        print(f"density {density}, skip {skip}: {int((host['n'] > 0).sum())} escaped pixels, worst {e.max():.4f} ulp(v)")
        worst = max(worst, float(e.max()))
    print(f"worst {worst:.4f} ulp(v); MEASURED_VALUE_ULPS_HOST {SM.MEASURED_VALUE_ULPS_HOST}")
    assert worst <= SM.MEASURED_VALUE_ULPS_HOST and SM.MEASURED_VALUE_ULPS_HOST - worst <= 0.1
    assert SM.VALUE_ULPS_GPU == SM.MEASURED_VALUE_ULPS_HOST + 1.0


def test_model_against_mpmath():
    cases = 0
    for (cr, ci), n_want in SM.TRUTH_POINTS:
        for s in SM.TRUTH_DENSITIES:
            p = SM.point(cr, ci, 5000, s)
            assert p["n"] == n_want, (cr, ci, p)
            agrees, truth = SM.hp_value(cr, ci, p["n"], p["N"], s, 0)
            assert agrees, (cr, ci, s)                      # count and run-on agree with mpmath
            err = abs(p["v"] - truth)
            measured = SM.MEASURED_TRUTH[((cr, ci), s)]
            print(f"c = {cr!r} + {ci!r}i, s {s}: n {p['n']}, N {p['N']}, v {p['v']!r}, error {err:.3e} (recorded {measured:.3e})")
            assert err <= 4.0 * measured, (cr, ci, s, err)
            assert _same(stripe_state_host((cr, ci), 5000, density=s), p)
            cases += 1
    assert cases == 9


def test_continuity_across_band_changes():
    """Along ci = 0.6, cr from 0.40463 to 0.404632, 2001 samples (spacing 1e-9), mrd 5000: the index N of the last point
    changes on the way.  Halving the spacing must not increase the largest difference between neighbours (a jump would stay), and
    at the density of the figures in the header's history (5) and below that difference is under 0.01.  The slope of
    sin(s arg z) grows with s, so at density 16 the 0.01 is not asked; there the largest difference must shrink to 0.6 of
    itself or less when the spacing halves, which a jump would not do."""
    cr = np.linspace(0.40463, 0.404632, 2001)
    for s in (1, 5, 16):
        px = [stripe_state_host((x, 0.6), 5000, density=s) for x in cr]
        v = np.array([p["v"] for p in px])
        assert len({p["N"] for p in px}) >= 2 and all(p["n"] > 0 for p in px)
        fine, coarse = np.abs(np.diff(v)).max(), np.abs(np.diff(v[::2])).max()
        print(f"density {s}: largest neighbour difference {fine:.3e} at spacing 1e-9, {coarse:.3e} at 2e-9")
        assert fine <= coarse
        if s <= 5:
            assert fine < 0.01
        else:
            assert fine <= 0.6 * coarse
        st = SM.states(cr, np.full(cr.size, 0.6), 5000, s, 0)
        assert np.array_equal(_bits(np.array([p["S"] for p in px])), _bits(st["S"])) and np.array_equal([p["N"] for p in px], st["N"])


def test_shade_host_equals_the_model():
    rng = np.random.default_rng(8)
    k = 4000
    v = rng.uniform(0.0, 1.0, k)
    v[::13] = 0.5
    v[1::17] = 0.0
    v[2::19] = 1.0
    v[3::23] = rng.uniform(-0.5, 1.5, v[3::23].size)      # outside [0, 1]: rounding can take a term past 1
    lo = np.where(rng.random(k) < 0.2, 0.0, rng.uniform(0.0, 1.0, k))
    lo[4::29] = 1.0
    gain = np.where(rng.random(k) < 0.2, 0.0, np.exp2(rng.uniform(-6.0, 10.0, k)))
    gain[5::31] = 2.0 ** 10
    gain[6::37] = 1.0
    got = np.array([stripe_shade_host(*(float(x) for x in s)) for s in zip(v, lo, gain)], np.int64)
    want = np.array([int(SM.shade(a, b, c)) for a, b, c in zip(v, lo, gain)], np.int64)
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 256 and len(np.unique(got)) > 200
    # by hand
    assert stripe_shade_host(0.5, 0.0, 1.0) == 128 and stripe_shade_host(1.0, 0.0, 1.0) == 256 and stripe_shade_host(0.0, 0.0, 1.0) == 0
    assert stripe_shade_host(0.75, 0.5, 1.0) == 224                  # w = 0.75, t = 0.5 + 0.5 * 0.75
    assert stripe_shade_host(0.75, 0.0, 4.0) == 256 and stripe_shade_host(0.25, 0.0, 4.0) == 0      # w clamps
    for x in (0.0, 0.3, 0.5, 0.9, 1.0):
        assert stripe_shade_host(x, 1.0, 3.0) == 256                # lo = 1: the base colour unchanged
        for l in (0.0, 0.25, 0.35, 1.0):
            assert stripe_shade_host(x, l, 0.0) == SM.neutral(l) == min(256, math.floor(256.0 * (l + (1.0 - l) * 0.5)))


def _palette(n=37, scale=2.3, offset=0.4):
    rng = np.random.default_rng(n)
    return Palette(rng.integers(0, 256, size=(n, 4), dtype=np.uint8), inside=(9, 200, 31, 77), scale=scale, offset=offset)


def _samples(rng, hs, ws):
    counts = rng.integers(0, 60, size=(hs, ws)).astype(np.int32)
    counts[rng.random((hs, ws)) < 0.25] = 0
    nu = np.where(counts > 0, counts + rng.uniform(-1.0, 1.0, size=(hs, ws)), 0.0)
    v = np.where(counts > 0, rng.uniform(0.0, 1.0, size=(hs, ws)), 0.0)
    return counts, nu, v


@pytest.mark.parametrize("s", [1, 2, 3])
def test_resolve_host_equals_the_model(s):
    rng = np.random.default_rng(200 + s)
    w, h = 7, 5
    pal = _palette()
    counts, nu, v = _samples(rng, h * s, w * s)
    esc = counts > 0
    for lo, gain in ((0.35, 1.0), (0.0, 2.5), (0.6, 2.0 ** 10), (0.125, 0.5)):
        got = stripe_resolve_host(pal, s, w, h, counts=counts, smooth=nu, stripe=v, lo=lo, gain=gain)
        want = SM.render(pal.entries, pal.inside, pal.scale, pal.offset, lo, gain, s, counts, nu, v)
        assert np.array_equal(got, want), (s, lo, gain)
    smooth = resolve_host(pal, "smooth", s, w, h, counts=counts, smooth=nu)
    # lo = 1 gives the smooth render's bytes, whatever the gain
    for gain in (0.0, 1.0, 2.0 ** 10):
        assert np.array_equal(stripe_resolve_host(pal, s, w, h, counts=counts, smooth=nu, stripe=v, lo=1.0, gain=gain), smooth)
    # gain = 0 gives the neutral q everywhere: the image does not depend on v
    for lo in (0.0, 0.35):
        a = stripe_resolve_host(pal, s, w, h, counts=counts, smooth=nu, stripe=v, lo=lo, gain=0.0)
        b = stripe_resolve_host(pal, s, w, h, counts=counts, smooth=nu, stripe=np.where(esc, 0.5, 0.0), lo=lo, gain=0.0)
        assert np.array_equal(a, b)
        if s == 1:
            want = smooth.astype(np.int64)
            want[..., :3] = (want[..., :3] * SM.neutral(lo) + 128) >> 8
            want[~esc] = pal.inside
            assert np.array_equal(a, want) and esc.sum() > 10 and (~esc).sum() > 3
    if s == 1:      # `inside` is not shaded; alpha is the base's
        dark = stripe_resolve_host(pal, 1, w, h, counts=counts, smooth=nu, stripe=np.zeros_like(v), lo=0.0, gain=1.0)
        assert (dark[esc][:, :3] == 0).all() and np.array_equal(dark[esc][:, 3], smooth[esc][:, 3])
        assert (dark[~esc] == np.array(pal.inside, np.uint8)).all()


def test_host_refusals():
    lib = L.load()
    pal = _palette()
    w, h = 4, 3
    counts, nu, v = _samples(np.random.default_rng(1), h, w)
    out = np.full((h, w, 4), 0xAB, np.uint8)

    def call(spec, width=w, height=h, c=counts, x=nu, m=v, o=out):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return lib.mbk_stripe_resolve_host(C.byref(spec) if spec is not None else None, width, height, ptr(c), ptr(x), ptr(m), ptr(o))

    assert call(pal.stripe_spec(1)) == L.MBK_OK and not (out == 0xAB).all()
    out[:] = 0xAB
    bad = [pal.stripe_spec(s) for s in (0, 5, 6, 7, 9, 16)]
    bad += [pal.stripe_spec(1, density=d) for d in (0, 17, 2 ** 31)]
    bad += [pal.stripe_spec(1, skip=2 ** 31)]
    bad += [pal.stripe_spec(1, lo=x) for x in (-1e-300, -1.0, 1.0000001, math.nan, math.inf)]
    bad += [pal.stripe_spec(1, gain=x) for x in (-1e-300, -1.0, 2.0 ** 10 + 1.0, math.nan, math.inf)]
    bad += [Palette(pal.entries[:1], scale=1.0).stripe_spec(1)]
    bad += [Palette(pal.entries, scale=x).stripe_spec(1) for x in (0.0, -1.0, 2.0 ** 21, math.nan)]
    bad += [Palette(pal.entries, offset=x).stripe_spec(1) for x in (2.0 ** 21, math.nan)]
    no_palette = pal.stripe_spec(1)
    no_palette.palette = None
    bad.append(no_palette)
    for spec in bad:
        assert call(spec) == L.MBK_ERR_INVALID
    assert call(None) == L.MBK_ERR_INVALID
    ok = pal.stripe_spec(1)
    assert call(ok, c=None) == call(ok, x=None) == call(ok, m=None) == L.MBK_ERR_INVALID
    assert call(ok, width=0) == call(ok, height=0) == L.MBK_ERR_INVALID
    assert call(ok, o=None) == L.MBK_ERR_INVALID
    assert (out == 0xAB).all()                               # a refusal writes nothing
    # the edges of the ranges are inside them
    for spec in (pal.stripe_spec(1, density=1), pal.stripe_spec(1, density=16), pal.stripe_spec(1, skip=2 ** 31 - 1),
                 pal.stripe_spec(1, lo=0.0), pal.stripe_spec(1, lo=1.0), pal.stripe_spec(1, gain=0.0), pal.stripe_spec(1, gain=2.0 ** 10)):
        assert call(spec) == L.MBK_OK
    with pytest.raises(MbkError):
        stripe_resolve_host(pal, 1, w, h, counts=counts, smooth=nu, stripe=v, lo=-1.0)
    with pytest.raises(ValueError):
        stripe_resolve_host(pal, 2, w, h, counts=counts, smooth=nu, stripe=v)
    # the state twin: density, skip, mrd and the output pointer
    st = L.mbk_stripe_state()
    st.S = 7.0
    for args in ((0.3, 0.5, 100, 0, 0), (0.3, 0.5, 100, 17, 0), (0.3, 0.5, 100, 5, 2 ** 31), (0.3, 0.5, 2 ** 31, 5, 0)):
        assert lib.mbk_stripe_state_host(*args, C.byref(st)) == L.MBK_ERR_INVALID and st.S == 7.0
    assert lib.mbk_stripe_state_host(0.3, 0.5, 100, 5, 0, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        stripe_state_host((0.3, 0.5), 100, density=17)
    # the device calls without a ctx, a value or a spec: refused before anything else is looked at
    view = L.mbk_view()
    buf = np.zeros(64)
    assert lib.mbk_view_launch_stripe(None, C.byref(view), 100, 0, 5, 0, None, buf.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_view_compute_stripe(None, C.byref(view), 100, 0, 5, 0, None, buf.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert lib.mbk_view_stripe_render_launch(None, C.byref(view), 100, 0, C.byref(ok), buf.ctypes.data, None) == L.MBK_ERR_INVALID
    assert lib.mbk_view_stripe_render_compute(None, C.byref(view), 100, 0, C.byref(ok), buf.ctypes.data, None) == L.MBK_ERR_INVALID
    assert not buf.any()


def test_struct_layouts():
    # uint32, pointer, uint32, uint8[4], two doubles, two uint32, two doubles, uint32 (+ tail padding): the header's field order
    assert C.sizeof(L.mbk_stripe_spec) == 8 + 8 + 4 + 4 + 2 * 8 + 2 * 4 + 2 * 8 + 8
    assert L.mbk_stripe_spec.density.offset == 40 and L.mbk_stripe_spec.lo.offset == 48 and L.mbk_stripe_spec.max_band_rows.offset == 64
    assert C.sizeof(L.mbk_stripe_state) == 48 and L.mbk_stripe_state.n.offset == 32
