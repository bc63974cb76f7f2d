"""Exterior distance estimates (include/mbk.h, "Distance estimates"), the parts that need no GPU: the numpy model of the
contract against Koebe's quarter theorem and against the same recurrences at 256 bits, the output expression
(mbk_distance_value_host, compiled from the function the kernel uses) against mpmath, and the colour rule of
MBK_RENDER_DISTANCE (mbk_render_resolve_host) against its numpy restatement.

Measured here (x86-64, glibc):
    Koebe      tip c = -2 - t: de / t in [3.885, 3.99999]; cusp c = 0.25 + t: [0.0018, 0.60]; c = -0.75 + i t: <= 0.029
    derivative worst relative error of the binary64 de against 256 bits 8.97e-7 at n = 127 (committed bound 3.6e-6,
               distance_model.py); no sample of any case is left out (count and run-on length agree everywhere)
    expression worst 1.941 ulp(de) (distance_model.D0 = 1.95)
"""
import ctypes as C
import math

import numpy as np
import pytest

import distance_model as M
import render_model as R
import smooth_truth as T
from distributedmandelbrot_amd import MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import resolve_host

TS = np.logspace(-6, -1, 300)
KOEBE = 4.0 * (1.0 + 2.0 ** -10)
MRD_LINES = 3_300_000        # pi / t steps at t = 1e-6 on the imaginary line


def _line(cr, ci, mrd=MRD_LINES):
    st = M.states(cr, ci, mrd)
    assert (st["n"] > 0).all(), "mrd too small: a sample of the line did not escape"
    return M.value(st["mag"], st["dmag"], st["n"]), st


def test_koebe_bound_on_the_antenna_tip():
    """c = -2 - t, nearest point of the set m = -2: de <= 4 t (1 + 2^-10), and the run-on makes it tight: de >= 3.8 t.
    Evaluated at the step that trips `>= 4`, or with the run-on capped at 8 steps, the upper bound fails by factors of
    4.7 to 2e5."""
    cr = -2.0 - TS
    de, st = _line(cr, np.zeros_like(cr), 1000)
    dist = np.abs(cr - (-2.0))                      # (of the binary64 sample, not of t)
    ratio = de / dist
    print(f"tip: de / distance in [{ratio.min():.6f}, {ratio.max():.6f}], run-on steps up to {st['extra'].max()}")
    assert (de <= KOEBE * dist).all(), float(ratio.max())
    assert (de >= 3.8 * dist).all(), float(ratio.min())
    assert st["extra"].max() > 8                    # the cap of 64 is needed here


def test_koebe_bound_on_the_cusp():
    """c = 0.25 + t, m = 0.25: one-sided (the estimate is known to undershoot next to a cusp)."""
    cr = 0.25 + TS
    de, _ = _line(cr, np.zeros_like(cr), 100000)
    dist = np.abs(cr - 0.25)
    ratio = de / dist
    print(f"cusp: de / distance in [{ratio.min():.6f}, {ratio.max():.6f}]")
    assert (de > 0).all() and (de <= KOEBE * dist).all(), float(ratio.max())


def test_koebe_bound_on_the_imaginary_line():
    """c = -0.75 + i t, m = -0.75 (the neck between the cardioid and the period-2 disc; ~pi / t steps to escape)."""
    de, st = _line(np.full_like(TS, -0.75), TS.copy())
    ratio = de / TS
    print(f"neck: de / distance in [{ratio.min():.6f}, {ratio.max():.6f}], counts up to {st['n'].max()}")
    assert (de > 0).all() and (de <= KOEBE * TS).all(), float(ratio.max())


# The plain small cases whose derivative is held to 256 bits: every SMALL_CASES entry whose coordinates mpmath can take as
# they are and whose escaped samples are a handful of thousands.  Left out: "huge" and "2^499" (n = 1 everywhere and mag
# overflows: nothing for a derivative to show; the expression test holds their values).
DERIVATIVE_CASES = [c for c in T.SMALL_CASES if c[0] not in ("huge", "2^499")]


def test_derivative_against_256_bits():
    """Same recurrences from the same binary64 c with mpmath at 256 bits: where the high-precision orbit escapes at the
    model's step and runs on as long, the model's de is within distance_model.DERIVATIVE_REL (relative).  The share of escaped
    samples left out because count or run-on length differ stays <= 1 % per case."""
    worst, worst_at = 0.0, None
    for name, v, mrd, window in DERIVATIVE_CASES:
        de, n, st = M.model(v, mrd, window)
        cr, ci = M.axes(v, window)
        crf, cif = np.tile(cr, ci.size), np.repeat(ci, cr.size)
        esc = np.flatnonzero(st["n"] > 0)
        out = 0
        case_worst = 0.0
        for i in esc:
            ok, hp = M.hp_sample(crf[i], cif[i], st["n"][i], st["extra"][i])
            if not ok:
                out += 1
                continue
            got = de.ravel()[i]
            if hp == 0.0 or not math.isfinite(hp):
                assert got == hp, (name, int(i))
                continue
            rel = abs(got - hp) / hp
            case_worst = max(case_worst, rel)
            if rel > worst:
                worst, worst_at = rel, (name, int(i), int(st["n"][i]))
        share = out / max(esc.size, 1)
        print(f"{name}: {esc.size} escaped, {out} left out ({100 * share:.2f} %), worst relative error {case_worst:.3e}")
        assert share <= 0.01, (name, share)
        assert case_worst <= M.DERIVATIVE_REL, (name, case_worst)
    print(f"derivative: worst relative error {worst:.3e} at {worst_at}; bound {M.DERIVATIVE_REL:.1e}")
    assert worst > 0.0


def _host_value(mag, dmag, n):
    f = L.load().mbk_distance_value_host
    return np.array([f(float(a), float(b), int(c)) for a, b, c in zip(mag, dmag, n)], np.float64)


EXPRESSION_CASES = [c for c in T.SMALL_CASES if c[0] in ("65x17", "win-0-0-77-53", "tiny-i", "ring", "far", "huge", "2^499")]


def test_output_expression_against_mpmath():
    """mbk_distance_value_host on the model's exact (mag, dmag) pairs against the correctly rounded value: within
    distance_model.D0 ulp(de), which is at most 0.1 above what this test measures; the special cases as the header lists them."""
    f = L.load().mbk_distance_value_host
    inf, nan = math.inf, math.nan
    assert f(16.0, 4.0, 0) == 0.0 and f(inf, 1.0, 0) == 0.0 and f(nan, nan, 0) == 0.0          # never escaped
    assert f(inf, 1.0, 1) == inf and f(inf, 1e300, 3) == inf                                   # mag overflowed
    assert f(2.0 ** 40, inf, 5) == 0.0                                                          # dmag overflowed
    assert f(inf, inf, 2) == 0.0 and f(2.0 ** 40, nan, 2) == 0.0 and f(nan, 1.0, 2) == 0.0      # NaN is stored as 0
    assert f(2.0 ** 40, 0.0, 2) == inf                                                          # dmag = 0
    assert f(4.0, 1.0, 1) == 2.0 * math.log(4.0)
    worst = 0.0
    for name, v, mrd, window in EXPRESSION_CASES:
        _, _, st = M.model(v, mrd, window)
        got = _host_value(st["mag"], st["dmag"], st["n"])
        assert not np.isnan(got).any() and (got[st["n"] == 0] == 0.0).all(), name
        worst = max(worst, M.assert_expression_within(got, st, name, M.D0))
        share = M.assert_states_agree(got, st, name)          # (numpy's ln against glibc's: the states are the same)
        print(f"{name}: {100 * share:.2f} % equal to the numpy model bit for bit")
        if name == "huge":
            assert np.isinf(got).any() and np.isfinite(got).any() and (got[np.isinf(st["mag"])] == inf).all()
        if name == "2^499":
            assert (got == inf).all()
    print(f"expression: worst {worst:.4f} ulp(de); D0 = {M.D0}")
    assert worst <= M.D0 <= worst + 0.1


def _palette(n, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=(n, 4)).astype(np.uint8)


@pytest.mark.parametrize("s", R.SUPERSAMPLES)
def test_colour_rule_against_the_numpy_model(s):
    """mbk_render_resolve_host with MBK_RENDER_DISTANCE, bit for bit: the clamp at n - 1, +inf, negative t, count 0, scales
    from pitch-relative 2^60 down to 1e-3, palettes of 2 to 65536 entries."""
    rs = np.random.RandomState(40 + s)
    w, h = 23, 11
    px = w * h * s * s
    for n, scale, offset in [(2, 1.0, 0.0), (7, 2.0 ** 60, -0.5), (256, 255 / 8e-3, 0.0), (65536, 1e3, 100.0), (16, 1e-3, 0.25),
                             (5, 2.0 ** 80, 0.0)]:
        pal = Palette(_palette(n, n), inside=(1, 2, 3, 4), scale=scale, offset=offset)
        de = np.abs(rs.standard_normal(px)) * (n / scale) * rs.choice([0.01, 0.5, 1.0, 2.0], size=px)
        de[rs.rand(px) < 0.05] = math.inf
        de[rs.rand(px) < 0.05] = 0.0
        de[rs.rand(px) < 0.03] = -1.0                  # (no launch stores one; the rule still says t = 0)
        de[::17] = (n - 1 - offset) / scale            # the clamp's edge
        de[1::17] = np.nextafter((n - 1 - offset) / scale, 0.0)
        counts = rs.randint(0, 5, size=px).astype(np.int32)
        want = M.render_distance(pal.entries, pal.inside, scale, offset, s, counts.reshape(h * s, w * s), de.reshape(h * s, w * s))
        got = resolve_host(pal, "distance", s, w, h, counts=counts, smooth=de)
        assert np.array_equal(got, want), (n, scale, offset, int((got != want).sum()))
    # NaN-free: a NaN handed in (no launch stores one) is t = 0, like a negative
    pal = Palette(_palette(4, 1), scale=1.0)
    got = resolve_host(pal, "distance", 1, 2, 1, counts=np.array([1, 1], np.int32), smooth=np.array([math.nan, -3.0]))
    assert np.array_equal(got[0, 0], pal.entries[0]) and np.array_equal(got[0, 1], pal.entries[0])


def test_colour_rule_refusals():
    counts, de = np.ones(4, np.int32), np.ones(4)
    ok = Palette(_palette(8, 2), scale=1.0)
    resolve_host(ok, "distance", 1, 2, 2, counts=counts, smooth=de)
    resolve_host(Palette(ok.entries, scale=2.0 ** 80), "distance", 1, 2, 2, counts=counts, smooth=de)
    for bad in (Palette(_palette(1, 3)), Palette(ok.entries, scale=0.0), Palette(ok.entries, scale=2.0 ** 81),
                Palette(ok.entries, scale=math.inf), Palette(ok.entries, scale=math.nan), Palette(ok.entries, offset=2.0 ** 21),
                Palette(_palette(65537, 4))):
        with pytest.raises(MbkError):
            resolve_host(bad, "distance", 1, 2, 2, counts=counts, smooth=de)
    with pytest.raises(MbkError):
        resolve_host(ok, "distance", 5, 2, 2, counts=np.ones(100, np.int32), smooth=np.ones(100))
    with pytest.raises(MbkError):
        resolve_host(ok, "distance", 1, 2, 2, counts=counts)                    # no de
    # smooth's own validation is untouched: its scale stops at 2^20
    with pytest.raises(MbkError):
        resolve_host(Palette(ok.entries, scale=2.0 ** 21), "smooth", 1, 2, 2, counts=counts, smooth=de)
    assert L.RENDER_SOURCES["distance"] == 3 == L.MBK_RENDER_DISTANCE


def test_palette_distance_helper():
    """Palette.distance(view, 8, inner_px=1): black within 1 px of the set, white beyond 8, one call."""
    view = View(-2.0, -1.5, 3.0, 3.0, 1025, 1025)
    pitch = 3.0 / 1024
    pal = Palette.distance(view, 8.0, inner_px=1.0)
    assert len(pal) == 256 and tuple(pal.entries[0]) == (0, 0, 0, 255) and tuple(pal.entries[-1]) == (255, 255, 255, 255)
    de = np.array([0.5, 1.0, 4.5, 8.0, 50.0, math.inf]) * pitch
    got = resolve_host(pal, "distance", 1, 6, 1, counts=np.ones(6, np.int32), smooth=de)[0]
    assert (got[0, :3] == 0).all() and (got[1, :3] == 0).all() and (got[3, :3] == 255).all() and (got[4, :3] == 255).all()
    assert (got[5, :3] == 255).all() and 120 <= got[2, 0] <= 135
    plain = Palette.distance(view, 8.0)
    assert plain.scale == 255 / (8.0 * pitch) and plain.offset == 0.0
    with pytest.raises(ValueError):
        Palette.distance(view, 1.0, inner_px=1.0)

