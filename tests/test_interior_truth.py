"""The interior distance estimate held to the mathematics (tests/interior_truth.py): de = (1 - |lambda|^2) / |d lambda / dc| of
the attracting cycle's multiplier, evaluated with mpmath at 256 bits from the pixel's coordinate and its period alone -- none
of the contract's recurrences.  The numpy model and the host twin are held to it on every settled pixel of three views; the
period must be the exact minimal period of the cycle and the cycle attracting, with no pixel left out.

Measured (the test prints the figures): K = worst rel (1 - |lambda|^2) / (p 2^-52) is 13.03 over the 586 settled pixels of the
64 x 64 full view at mrd 1500, 20.13 over the 50 of the seahorse view at mrd 2000 (periods 27, 29, 58) and 68.52 over the 4002 of
the 160 x 160 grid at mrd 4096 (periods 1 to 29); the worst relative errors are 4.1e-14, 2.7e-13 and 2.0e-13.  The analytic
|F + E B / (1 - A)| agrees with the finite difference of the multiplier to 4.6e-39 relative at worst.

Run once against two mutations of interior_model.distance, and the first case failed at once under each: AB computed from the
new A (K 1.1e15 on the 64 x 64 full view, at a period-2 pixel) and the factor 2 of E dropped (K 1.2e16)."""
import numpy as np
import pytest

import interior_truth as T
from distributedmandelbrot_amd.device import interior_host

CASES = [("full64", T.FULL64), ("seahorse", T.SEAHORSE), ("grid160", T.GRID160)]
_K = {}


@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_model_equals_the_truth_on_every_settled_pixel(name, case):
    cr, ci, m = T.model_case(case)
    settled = m["period"] > 0
    assert int(settled.sum()) == {"full64": 586, "seahorse": 50, "grid160": 4002}[name]
    if name == "seahorse":
        assert sorted(np.unique(m["period"][settled])) == [27, 29, 58]
    if name == "grid160":
        assert (m["period"] > 2).sum() > 200 and m["period"].max() == 29
    w = T.assert_truth(cr, ci, m["period"], m["de"], case[1], name, with_analytic=True)
    assert w["settled"] == int(settled.sum())            # no pixel is left out
    assert w["worst_analytic"] <= 1e-30, name            # the contract's formula IS the derivative of the multiplier
    _K[name] = w["K"]


def test_k0_is_what_the_cases_measure():
    """K0 is a record of the measurement, not a margin: at most 10 % above the worst case."""
    for name, case in CASES:
        if name not in _K:
            cr, ci, m = T.model_case(case)
            _K[name] = T.measure(cr, ci, m["period"], m["de"], case[1], name)["K"]
    worst = max(_K.values())
    print(f"K per case {_K}, K0 {T.K0}")
    assert worst <= T.K0 <= 1.1 * worst


@pytest.mark.parametrize("name,case", CASES, ids=[c[0] for c in CASES])
def test_host_twin_equals_the_truth_on_a_sample(name, case):
    """The same truth through mbk_interior_host, with no model in between: 100 seeded settled pixels per case (every one of the
    seahorse view's 50)."""
    cr, ci, m = T.model_case(case)
    settled = np.flatnonzero(m["period"] > 0)
    pick = settled if settled.size <= 100 else np.sort(np.random.RandomState(7).choice(settled, 100, replace=False))
    got = [interior_host((float(cr[i]), float(ci[i])), case[1]) for i in pick]
    period = np.array([g[1] for g in got], np.int32)
    de = np.array([g[3] for g in got], np.float64)
    assert (np.array([g[0] for g in got]) == 0).all() and (period > 0).all()
    w = T.assert_truth(cr[pick], ci[pick], period, de, case[1], "host " + name)
    assert w["settled"] == pick.size
