"""The continuous escape-time value against the truth (CPU).  tests/smooth_truth.py evaluates
nu = n + 1 - log2(0.5 ln mag) with mpmath on the exact binary64 mag; here the two CPU references that judge the GPU --
the C oracle (glibc's log / log2) and tests/deep_model.smooth_from (numpy's) -- are measured against it on every view of
the GPU smooth tests, and the oracle's new mag output is proved against a plain scalar loop.

The worst figures of these references, A0 ulp(nu) where |nu| >= 1 and B0 x 2^-52 where |nu| < 1, are what the GPU's
bound is built from (smooth_truth.A0, .B0): test_reference_error_is_within_the_recorded_figures prints what this run
measured and fails if a case exceeds the recorded constants."""
import math

import mpmath
import numpy as np
import pytest

import deep_model as D
import smooth_truth as T

MEASURED = {}       # case name -> (A, A_at, B, B_at, err_abs, escaped pixels)


def _measure(name, got, counts, mag):
    w = T.assert_within(got, counts, mag, name, A=T.A0, B=T.B0)
    assert w["A"] <= T.A0 and w["B"] <= T.B0, (name, w["A"], w["A_at"], w["B"], w["B_at"])
    MEASURED[name] = (w["A"], w["A_at"], w["B"], w["B_at"], w["err_abs"], w["n_escaped"])
    return w


def test_nu_true_known_answers():
    d, v = T.nu_true(1, 4.0)                    # c = -2: z_1 = 2, mag = 4 exactly, nu = 2 - log2(ln 2)
    with mpmath.workprec(300):
        want = 2 - mpmath.log(mpmath.log(2), 2)
        assert abs(v - want) < mpmath.mpf(2) ** -240
    assert d == 2.5287663729448977 and abs(v - d) <= T.ulp(d) / 2
    assert T.nu_true(0, 123.0)[0] == 0.0 and T.nu_true(0, 0.0)[0] == 0.0
    assert T.nu_true(7, math.inf)[0] == -math.inf
    assert T.nu_true(3, math.e ** 2)[0] == pytest.approx(4.0, abs=1e-15)      # 0.5 ln mag = 1: nu = n + 1
    with pytest.raises(ValueError):
        T.nu_true(1, 3.9999)
    with pytest.raises(ValueError):
        T.nu_true(1, math.nan)
    # the nearest double really is the nearest: the rest is at most half an ulp, and the mpf does not move with precision
    for n, mag in [(1, 4.0), (1, 4.000000000000001), (12, 17.25), (4999, 5.5), (1, 1e305), (1, 2981.0)]:
        d, v = T.nu_true(n, mag)
        assert abs(v - mpmath.mpf(d)) <= mpmath.mpf(float(T.ulp(d))) / 2
        with mpmath.workprec(1000):
            hi = n + 1 - mpmath.log(mpmath.log(mpmath.mpf(mag)) / 2, 2)
        assert abs(hi - v) < mpmath.mpf(2) ** -230


def test_error_measure():
    near, rest = np.array([2.5, -math.inf, 1.0]), np.array([2.0 ** -55, 0.0, 0.0])
    e, eu = T.err(np.array([2.5 + 2.0 ** -51, -math.inf, math.nan]), near, rest)
    assert e[0] == 2.0 ** -51 - 2.0 ** -55 and eu[0] == e[0] / 2.0 ** -51
    assert e[1] == 0.0 and math.isinf(e[2])
    assert math.isinf(T.err(np.array([1e300]), np.array([-math.inf]), np.array([0.0]))[0][0])
    assert T.bound(np.array([2.5, -math.inf, 0.0]), 2, 3).tolist() == [2 * 2.0 ** -51 + 3 * 2.0 ** -52, 0.0, 0.0]


def test_oracle_mag_equals_a_plain_scalar_loop(oracle):
    """The oracle's mag output against calc_mb_value restated with numpy float64 scalars (which round every operation
    and never fuse): the count, and |z_n|^2 of the step that tripped `>= 4`, bit for bit; and a window equals the
    slice of the whole."""
    f = np.float64
    view, mrd = (-2.0, -1.25, 2.5, 2.5, 23, 17), 60
    sm, c, mag = oracle.view_smooth_mag(*view, mrd)
    xr, xi = oracle.axis(view[0], view[2], view[4]), oracle.axis(view[1], view[3], view[5])
    with np.errstate(over="ignore"):
        for r in range(view[5]):
            for k in range(view[4]):
                cr, ci = f(xr[k]), f(xi[r])
                zr, zi, n_esc, m_esc = cr, ci, 0, f(0.0)
                for n in range(1, mrd):
                    t = zr * zr - zi * zi
                    u = (f(2.0) * zr) * zi
                    zr, zi = t + cr, u + ci
                    m = zr * zr + zi * zi
                    if m >= 4.0:
                        n_esc, m_esc = n, m
                        break
                assert (c[r, k], mag[r, k]) == (n_esc, m_esc), (r, k)
    assert len(np.unique(c)) >= 8 and (c == 0).any()
    sm2, c2 = oracle.view_smooth(*view, mrd)
    assert np.array_equal(sm, sm2) and np.array_equal(c, c2)
    assert all(sm[r, k] == oracle.smooth_value(c[r, k], mag[r, k]) for r in range(17) for k in range(23))
    w = (3, 2, 11, 9)
    smw, cw, magw = oracle.view_smooth_mag(*view, mrd, window=w)
    assert np.array_equal(smw, sm[2:11, 3:14]) and np.array_equal(cw, c[2:11, 3:14]) and np.array_equal(magw, mag[2:11, 3:14])
    c0, _, _ = oracle.view(*view, mrd, want_bytes=False)
    assert np.array_equal(c, c0)


@pytest.mark.parametrize("name, view, mrd, window", T.SMALL_CASES, ids=[c[0] for c in T.SMALL_CASES])
def test_oracle_against_truth_small_views(oracle, name, view, mrd, window):
    sm, c, mag = oracle.view_smooth_mag(*view, mrd, window=window)
    assert not np.isnan(sm).any()
    w = _measure(name, sm, c, mag)
    if name == "ring":
        assert (c[16, 0], mag[16, 0]) == (1, 4.0) and sm[16, 0] == T.nu_true(1, 4.0)[0] == 2.5287663729448977
    if name == "huge":
        fin = np.isfinite(mag)
        assert (c == 1).all() and fin.any() and (~fin).any() and mag[fin].max() > 1e305
        assert (sm[~fin] == -math.inf).all() and np.isfinite(sm[fin]).all()
    if name == "2^499":
        assert (c == 1).all() and np.isinf(mag).all() and (sm == -math.inf).all()
    if name == "far":
        near = w["near"]
        assert (np.abs(near) < 1).sum() >= 20 and (near < 0).any() and (near > 0).any()


SMOOTH_PARITY_VIEWS = [((-2.0, -1.5, 3.0, 3.0, 512, 512), 5000), ((-0.755, 0.10, 0.02, 0.02, 300, 200), 5000),
                       ((-0.755, 0.10, 0.02, 0.02, 700, 500), 900), ((-0.3, -0.2, 0.7, 0.4, 200, 160), 2500)]


@pytest.mark.parametrize("view, mrd", SMOOTH_PARITY_VIEWS)
def test_oracle_against_truth_parity_views(oracle, view, mrd):
    """The views of the smooth asserts in tests/test_gpu_parity.py that have escaped pixels (two lie wholly inside the
    set), on a seeded sample of 4 000 escaped pixels each."""
    sm, c, mag = oracle.view_smooth_mag(*view, mrd)
    esc = np.flatnonzero(c.ravel() > 0)
    assert esc.size >= 100
    pick = np.random.RandomState(3).choice(esc, min(4000, esc.size), replace=False)
    _measure("parity-%gx%d" % (view[2], view[4]), sm.ravel()[pick], c.ravel()[pick], mag.ravel()[pick])


def test_oracle_against_truth_cfg5_sample(oracle):
    """BASELINE cfg5 at full size: the sample the GPU test checks (20 000 seeded escaped pixels, the 1 000 largest and
    the 1 000 smallest mag)."""
    sm, c, mag = T.cfg5_oracle(oracle)
    pick = T.cfg5_sample(c, mag)
    assert 21000 <= pick.size <= 22000
    _measure("cfg5", sm.ravel()[pick], c.ravel()[pick], mag.ravel()[pick])


@pytest.mark.parametrize("case", T.DEEP_CASES, ids=["%s-%g" % (c[0][0][:8], c[1]) for c in T.DEEP_CASES])
def test_deep_model_smooth_against_truth(case):
    orbit, view, mrd, window, c, mag = T.deep_model_case(case)
    sm = D.smooth_from(c, mag)
    esc = np.flatnonzero(c.ravel() > 0)
    assert esc.size
    pick = np.random.RandomState(4).choice(esc, min(4000, esc.size), replace=False)
    _measure("deep-%s-%g-%s" % (case[0][0][:8], case[1], case[2]), sm.ravel()[pick], c.ravel()[pick], mag.ravel()[pick])
    if case[0] == ("-2", "0"):
        assert orbit.length == 1 and orbit.escaped


def _sweep(top, extra=()):
    """Doubles from 4.0 to top: 4.0 and its next neighbours, then 4 000 points spread evenly in log(mag), then
    `extra` = (lo, hi, count) stretches sampled more densely."""
    first = [4.0]
    for _ in range(8):
        first.append(float(np.nextafter(first[-1], np.inf)))
    parts = [first, np.exp(np.linspace(np.log(4.0), np.log(top), 4000))[1:-1], [top]]
    parts += [np.exp(np.linspace(np.log(lo), np.log(hi), k)) for lo, hi, k in extra]
    return np.unique(np.concatenate(parts))


def _check_sweep(oracle, n, mags, measured):
    counts = np.full(mags.shape, n, np.int32)
    got = np.array([oracle.smooth_value(n, m) for m in mags])
    near, rest = T.nu_true_array(counts, mags)
    if measured:
        w = _measure("sweep-n%d" % n, got, counts, mags)
        assert np.array_equal(w["near"], near)
    hp = [T.nu_true(n, m)[1] for m in mags[:40]]
    assert all(a > b for a, b in zip(hp, hp[1:]))               # strictly, in the high-precision values
    assert (np.diff(near) <= 0).all() and near[0] > near[-1]
    return got, near, rest


def test_formula_sweep_of_mag_at_n_1(oracle):
    """n = 1 is the only count at which mag is unbounded (|c| > 2 gives |z_1| >= |c| (|c| - 1) > 2).  Over mag from 4.0
    to 1e300, 4.0 + 1 ulp included: the truth decreases strictly in mag, its nearest double never increases, the oracle's
    value does not increase beyond the two bounds, and the oracle is within (A0, B0).  nu passes through 0 at mag = e^8,
    where ulp(nu) vanishes and only the absolute term holds; the stretch e^4 .. e^32, where ulp(L) is 2 to 4 times
    ulp(nu), is sampled densely."""
    mags = _sweep(1e300, extra=[(math.e ** 4, math.e ** 16, 10000), (math.e ** 16, math.e ** 32, 10000)])
    assert mags[0] == 4.0 and mags[1] == 4.0 + 2.0 ** -50 and mags[-1] == 1e300
    got, near, _ = _check_sweep(oracle, 1, mags, True)
    slack = T.bound(near, T.A0, T.B0)
    assert (np.diff(got) <= slack[1:] + slack[:-1]).all()
    assert near[0] == 2.5287663729448977 and (np.abs(near) < 1).sum() > 5000 and near[-1] < -6
    assert oracle.smooth_value(1, math.inf) == -math.inf == T.nu_true(1, math.inf)[0]
    assert oracle.smooth_value(0, 5.0) == 0.0


@pytest.mark.parametrize("n", [2, 9, 1000, 4999])
def test_formula_sweep_of_mag(oracle, n):
    """n >= 2: |z_(n-1)| < 2 and |c| <= 2 (or n would be 1), so |z_n| <= 6 and mag <= 36.  The sweep that is measured
    against (A0, B0) runs from 4.0 to 40; monotonicity of the truth is checked up to 1e300 all the same (the formula does
    not know where mag came from), without an error bound, which up there would measure log2's ulp at |L| ~ 9 against
    ulp(nu) of a pixel that cannot exist."""
    mags = _sweep(40.0)
    assert mags[0] == 4.0 and mags[1] == 4.0 + 2.0 ** -50 and mags[-1] == 40.0
    got, near, _ = _check_sweep(oracle, n, mags, True)
    slack = T.bound(near, T.A0, T.B0)
    assert (np.diff(got) <= slack[1:] + slack[:-1]).all()
    assert n + 1 - 1.25 < near[-1] < near[0] == T.nu_true(n, 4.0)[0]
    _check_sweep(oracle, n, _sweep(1e300)[::4], False)
    assert oracle.smooth_value(n, math.inf) == -math.inf == T.nu_true(n, math.inf)[0]


def test_reference_error_is_within_the_recorded_figures():
    """Runs last in this module: the worst of every case above.  A0 / B0 in smooth_truth.py are these figures rounded
    up; the GPU tests allow A0 + 1 and B0 + 2."""
    complete = len(MEASURED) == len(T.SMALL_CASES) + len(SMOOTH_PARITY_VIEWS) + 1 + len(T.DEEP_CASES) + 5
    a = max(MEASURED.items(), key=lambda kv: kv[1][0])
    b = max(MEASURED.items(), key=lambda kv: kv[1][2])
    e = max(MEASURED.items(), key=lambda kv: kv[1][4])
    total = sum(v[5] for v in MEASURED.values())
    print(f"\nCPU references against nu_true over {len(MEASURED)} cases, {total} escaped pixels:")
    print(f"  A0 measured {a[1][0]:.4f} ulp(nu)  in {a[0]} at (index, n, mag) {a[1][1]}   [recorded {T.A0}]")
    print(f"  B0 measured {b[1][2]:.4f} x 2^-52  in {b[0]} at (index, n, mag) {b[1][3]}   [recorded {T.B0}]")
    print(f"  worst err_abs {e[1][4]:.3e} in {e[0]}")
    assert a[1][0] <= T.A0 and b[1][2] <= T.B0
    if complete:        # every case of this module ran: the recorded figures are not looser than what is measured
        assert a[1][0] > T.A0 - 0.1 and b[1][2] > T.B0 - 0.1
