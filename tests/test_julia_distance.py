"""Distance estimates for Julia views (include/mbk.h, the section of that name), the parts that need no GPU: the host twin
(mbk_julia_distance_host, compiled from the step function the kernels use) against the numpy model of the contract
(tests/julia_distance_model.py), the model against the same recurrences at 256 bits, the output expression on Julia pairs
against mpmath, and geometry whose answer is known in closed form.

Measured here (x86-64, glibc):
    host twin   every state bit of every sample of every small case equals the model's
    derivative  worst relative error of the binary64 de against 256 bits 1.314e-1, at a sample within an ulp of the unit
                circle (committed bound 0.8, julia_distance_model.py, which lists the figure of each case); two samples in all
                are left out (count or run-on length differ)
    expression  worst 2.0018 ulp(de) (julia_distance_model.J0 = 2.01)
    geometry    c = 0: |de / (2 |p| ln |p|) - 1| <= 5.8e-14; c = -2: de / t in [3.99999997, 4.0033] left of the tip and in
                [2.0000, 2.00002] above 0.5; on the grid de / distance in [2.0, 4.16]
"""
import ctypes as C
import math

import numpy as np
import pytest

import julia_distance_model as JM
import julia_model as J
from distributedmandelbrot_amd import MbkError
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import device as Dv

STATE_KEYS = ("zr", "zi", "dr", "di", "mag", "dmag")


def _host_states(zr0, zi0, c, mrd):
    """mbk_julia_distance_host on flat arrays of starting points: the model's dict, plus de."""
    out = {k: np.empty(zr0.size, np.int32) for k in ("n", "extra")}
    out.update({k: np.empty(zr0.size, np.float64) for k in STATE_KEYS + ("de",)})
    for j in range(zr0.size):
        r = Dv.julia_distance_host((zr0[j], zi0[j]), c, mrd)
        for k, a in out.items():
            a[j] = r[k]
    return out


_HOST = {}


def _host_case(case):
    name, v, c, mrd, window = case
    if name not in _HOST:
        _HOST[name] = _host_states(*JM.points(v, window), c, mrd)
    return _HOST[name]


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("case", JM.SMALL_CASES, ids=[c[0] for c in JM.SMALL_CASES])
def test_host_twin_equals_the_model_on_every_state_bit(case):
    """n, extra, z, d, mag, dmag bit for bit; de through the ln candidates (glibc's ln against numpy's).  The counts are
    those of the Julia count contract (tests/julia_model.py)."""
    name, v, c, mrd, window = case
    mde, mn, st = JM.case_model(case)
    got = _host_case(case)
    assert np.array_equal(got["n"], st["n"]) and np.array_equal(got["extra"], st["extra"]), name
    for k in STATE_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(st[k])), (name, k, int((_bits(got[k]) != _bits(st[k])).sum()))
    n_count, _ = J.julia_view(v, c, mrd, window)
    assert np.array_equal(mn, n_count), name
    assert not np.isnan(got["de"]).any() and (got["de"] >= 0.0).all() and np.array_equal(got["de"] == 0.0, got["n"] == 0), name
    share = JM.assert_states_agree(got["de"], st, name)
    print(f"{name}: {100 * share:.2f} % of de equal to the numpy model bit for bit")
    if name == "2^499":
        assert (got["de"] == math.inf).all() and (got["n"] == 1).all()
    if name == "far":       # |c| > 2: the run-on is short, and the literal facts the issue records
        esc = st["n"] > 0
        assert esc.all() and st["extra"][esc].min() == 3 and st["extra"][esc].max() == 5
    if name == "neck":
        assert int((st["n"] == 0).sum()) == 1067
    if name == "dust":
        assert int(st["n"].max()) == 771


def test_model_against_256_bits():
    """The same two recurrences from the same binary64 z_0 and c with mpmath at 256 bits: where the high-precision orbit
    escapes at the model's step and runs on as long, the model's de is within julia_distance_model.DERIVATIVE_REL (relative).
    At least 99 % of the escaped samples of each case take part."""
    worst, worst_at = 0.0, None
    for case in JM.DERIVATIVE_CASES:
        name, v, c, mrd, window = case
        de, n, st = JM.case_model(case)
        zr0, zi0 = JM.points(v, window)
        esc = np.flatnonzero(st["n"] > 0)
        out, case_worst = 0, 0.0
        for i in esc:
            ok, hp = JM.hp_sample(zr0[i], zi0[i], c, st["n"][i], st["extra"][i])
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
        assert case_worst <= JM.DERIVATIVE_REL, (name, case_worst)
    print(f"derivative: worst relative error {worst:.3e} at {worst_at}; bound {JM.DERIVATIVE_REL:.1e}")
    assert worst > 0.0


def test_output_expression_against_mpmath():
    """The host twin's de on the model's exact Julia (mag, dmag) pairs against the correctly rounded value: within
    julia_distance_model.J0 ulp(de), which is at most 0.1 above what this test measures."""
    worst = 0.0
    for case in JM.SMALL_CASES:
        name = case[0]
        _, _, st = JM.case_model(case)
        got = _host_case(case)["de"]
        worst = max(worst, JM.assert_expression_within(got, st, name, JM.J0))
    print(f"expression: worst {worst:.4f} ulp(de); J0 = {JM.J0}")
    assert worst <= JM.J0 <= worst + 0.1


def test_unit_circle_has_the_closed_form():
    """c = 0: z_k = p^(2^k), d_k = 2^k p^(2^k - 1), so de = 2 |p| ln |p| whatever the step it is read at."""
    case = JM.SMALL_CASES[0]
    name, v, c, mrd, window = case
    assert c == (0.0, 0.0)
    de, n, st = JM.case_model(case)
    host = _host_case(case)["de"]
    zr0, zi0 = JM.points(v, window)
    r = np.hypot(zr0, zi0)
    pick = r > 1.001
    assert int(pick.sum()) == 2456 and int((st["n"] == 0).sum()) == 1623
    want = 2.0 * r[pick] * np.log(r[pick])
    for what, got in (("model", de.ravel()), ("host", host)):
        rel = np.abs(got[pick] / want - 1.0)
        print(f"c = 0 {what}: {int(pick.sum())} samples, worst |de / (2 |p| ln |p|) - 1| = {rel.max():.2e}")
        assert (rel <= 1e-12).all(), (what, float(rel.max()))


TS = np.logspace(-2, -12, 41)


def _line_host(zr0, zi0, c, mrd):
    st = _host_states(np.asarray(zr0, np.float64), np.asarray(zi0, np.float64), c, mrd)
    assert (st["n"] > 0).all(), "mrd too small: a sample of the line did not escape"
    return st["de"]


def test_segment_lines():
    """c = -2, the Julia set is the segment [-2, 2].  Left of the tip the distance of p = -2 - t is t and Koebe's 4 is attained;
    above an inner point, p = 0.5 + i t, the distance is t and the estimate reads 2 t."""
    c, mrd = (-2.0, 0.0), 4000
    for zr0, zi0, lo, hi, what in ((-2.0 - TS, np.zeros_like(TS), 3.99, 4.01, "tip"), (np.full_like(TS, 0.5), TS.copy(), 1.99, 2.01, "above 0.5")):
        dist = np.hypot(zr0 - np.clip(zr0, -2.0, 2.0), zi0)      # (of the binary64 sample, not of t)
        for name, de in (("model", None), ("host", _line_host(zr0, zi0, c, mrd))):
            if de is None:
                st = JM.states(zr0, zi0, c, mrd)
                assert (st["n"] > 0).all()
                de = JM.value(st["mag"], st["dmag"], st["n"])
            ratio = de / dist
            print(f"c = -2 {what} {name}: de / t in [{ratio.min():.8f}, {ratio.max():.8f}]")
            assert (ratio >= lo).all() and (ratio <= hi).all(), (what, name, float(ratio.min()), float(ratio.max()))


def test_segment_grid():
    """c = -2 on a grid around the segment: de / distance lies in [2.0, 4.16], and no escaped sample stores 0."""
    v, c, mrd = (-2.5, -1.0, 5.0, 2.0, 81, 41), (-2.0, 0.0), 2000
    de, n, st = JM.model(v, c, mrd)
    zr0, zi0 = JM.points(v)
    host = _host_states(zr0, zi0, c, mrd)
    assert np.array_equal(host["n"], st["n"])
    dist = np.hypot(zr0 - np.clip(zr0, -2.0, 2.0), zi0)
    esc = st["n"] > 0
    off = dist > 0.0
    # every sample off the segment escapes.  On it some do too: 0, -2 and 2 reach z = 2, where mag = 4 trips `>= 4`; z then
    # stays at 2 through the run-on and d keeps growing, so their de is tiny, but not 0
    assert esc[off].all() and (~off).any() and not esc[~off].all() and esc[~off].any()
    for what, got in (("model", de.ravel()), ("host", host["de"])):
        assert (got[esc] > 0.0).all() and not np.isnan(got).any(), what
        # (the grid's centre is the critical point, which reaches -2 at once: n = 1, d = 0, +inf)
        assert np.array_equal(np.isinf(got), (zr0 == 0.0) & (zi0 == 0.0)) and np.isinf(got).sum() == 1, what
        ratio = got[off] / dist[off]
        print(f"c = -2 grid {what}: {int(off.sum())} samples off the segment, de / distance in [{ratio.min():.6f}, {ratio.max():.6f}]")
        assert (ratio >= 2.0).all() and (ratio <= 4.16).all(), (what, float(ratio.min()), float(ratio.max()))


def test_the_critical_point_stores_infinity():
    """The centre pixel of the 65 x 65 view is z_0 = 0 exactly: d_k = 0 for every k >= 1, n = 19, dmag = 0, de = +inf -- and it
    is the only infinity in the view."""
    case = next(c for c in JM.SMALL_CASES if c[0] == "critical")
    name, v, c, mrd, window = case
    de, n, st = JM.case_model(case)
    zr0, zi0 = JM.points(v)
    centre = 32 * 65 + 32
    assert zr0[centre] == 0.0 and zi0[centre] == 0.0
    r = Dv.julia_distance_host((0.0, 0.0), c, mrd)
    assert r["n"] == 19 and r["dmag"] == 0.0 and r["dr"] == 0.0 and r["di"] == 0.0 and r["de"] == math.inf
    assert st["n"][centre] == 19 and st["dmag"][centre] == 0.0 and de.ravel()[centre] == math.inf
    host = _host_case(case)["de"]
    for got in (de.ravel(), host):
        assert np.flatnonzero(np.isinf(got)).tolist() == [centre]


def test_host_twin_refusals_and_trivial_depths():
    lib = L.load()
    f = lib.mbk_julia_distance_host
    n, x = C.c_int32(-7), C.c_int32(-7)
    vals = [C.c_double(-7.0) for _ in range(7)]
    ptrs = [C.byref(v) for v in vals]
    assert f(0.5, 0.5, 0.0, 1.0, 100, None, C.byref(x), *ptrs) == L.MBK_ERR_INVALID
    for bad in ((math.inf, 0.0), (0.0, math.nan), (-math.inf, math.nan)):
        assert f(0.5, 0.5, bad[0], bad[1], 100, C.byref(n), C.byref(x), *ptrs) == L.MBK_ERR_INVALID
        with pytest.raises(MbkError):
            Dv.julia_distance_host((0.5, 0.5), bad, 100)
    assert f(0.5, 0.5, 0.0, 1.0, 2 ** 31, C.byref(n), C.byref(x), *ptrs) == L.MBK_ERR_INVALID
    assert n.value == -7 and x.value == -7 and all(v.value == -7.0 for v in vals)        # nothing written
    assert f(0.5, 0.5, 0.0, 1.0, 2 ** 31 - 1, C.byref(n), C.byref(x), *ptrs) == L.MBK_OK
    # every output pointer but count may be NULL
    assert f(3.0, 0.0, 0.0, 1.0, 100, C.byref(n), None, None, None, None, None, None, None, None) == L.MBK_OK and n.value == 1
    for mrd in (0, 1):      # no step runs: the initial state, count and de 0
        r = Dv.julia_distance_host((3.0, -4.0), (0.0, 1.0), mrd)
        assert r == {"n": 0, "extra": 0, "zr": 3.0, "zi": -4.0, "dr": 1.0, "di": 0.0, "mag": 25.0, "dmag": 1.0, "de": 0.0}
        st = JM.states([3.0], [-4.0], (0.0, 1.0), mrd)
        assert st["n"][0] == 0 and st["mag"][0] == 25.0 and st["dmag"][0] == 1.0
    r = Dv.julia_distance_host((3.0, -4.0), (0.0, 1.0), 2)
    assert r["n"] == 1 and r["de"] > 0.0
