"""The deep-zoom contract against the truth (CPU): the numpy model of the step (tests/deep_model.py, what the GPU is held to
bit for bit) on the library's own orbit table, compared with z = z^2 + c iterated directly in fixed point at P + 128
fraction bits, over a seeded catalogue of centres, spans and mrds.  Every case has at least 8 distinct counts in the
truth, so none passes by being flat.  The tip of the antenna (c within ~1e-16 of -2) is a known limit of the contract and
is pinned as a strict xfail."""
import numpy as np
import pytest

import deep_model as D

# Misiurewicz points (preperiodic, on the boundary) to 40 digits: the truncated centres escape after a few hundred steps
M41 = ("-0.1010963638456221610257854457386225654638", "0.9562865108091415007710960577299774358098")
M51 = ("0.3663629834227643413289327307978490580499", "0.5915337732614452275774934937165419811535")

# (centre, span_r, span_i (None: square), mrd, the orbit's length M, escaped)
CASES = [
    (("-1.543689012692076361570855971", "0"), 1e-25, None, 3000, 3000, False),   # Misiurewicz, c^3 + 2c^2 + 2c + 2 = 0
    (("0", "1"), 1e-30, None, 3000, 3000, False),
    (("-0.75", "0"), 1e-25, 4e-3, 5000, 5000, False),   # root of the period-2 bulb: counts ~ pi / |Im dc|
    (("0.25", "0"), 2e-4, 1e-30, 5000, 5000, False),    # the cusp: counts ~ pi / sqrt(Re dc)
    (("1e-21", "1"), 1e-20, None, 5000, 58, True),
    (("-0.77568377", "0.13646737"), 1e-12, None, 3000, 447, True),
    (M41, 1e-25, None, 3000, 338, True),
    (M51, 1e-35, None, 3000, 502, True),
    (("-2", "0"), 1e-10, None, 1000, 1, True),
]

TIP = pytest.mark.xfail(strict=True, raises=AssertionError,
                        reason="the orbit table holds Z_m rounded to binary64: within ~1e-16 of -2 the real orbit stays "
                               "just inside |z| = 2, the table holds 2.0 and every pixel retires at count 1 "
                               "(a wider table is a separate ABI change)")
TIP_CASES = [
    pytest.param(("-2", "0"), 1e-30, None, 3000, 1, True, marks=TIP, id="tip-2-1e-30"),
    pytest.param(("-1.9999999999999999999999999999", "0"), 1e-35, None, 3000, 3000, False, marks=TIP, id="tip-2+1e-28-1e-35"),
]


def _sample(centre, span_r, span_i, mrd, n=64, pixels=150, seed=1):
    from distributedmandelbrot_amd import DeepOrbit, DeepView
    orbit = DeepOrbit(*centre, mrd, min_span=min(span_r, span_i or span_r))
    view = DeepView(span_r, n, n, span_i)
    dr, di = D.offsets(view)
    pick = np.random.RandomState(seed).choice(dr.size, pixels, replace=False)
    return orbit, dr[pick], di[pick]


@pytest.mark.parametrize("centre, span_r, span_i, mrd, M, escaped", CASES + TIP_CASES)
def test_model_equals_direct_iteration(centre, span_r, span_i, mrd, M, escaped):
    orbit, dr, di = _sample(centre, span_r, span_i, mrd)
    assert (orbit.length, orbit.escaped) == (M, escaped)
    zr, zi = orbit.table()
    model, _ = D.model_counts(zr, zi, dr, di, mrd)
    truth = D.direct_counts(centre[0], centre[1], dr, di, mrd, orbit.precision_bits + 128)
    assert len(np.unique(truth)) >= 8, np.unique(truth)
    assert (model == truth).mean() >= 0.99, (int((model != truth).sum()), np.unique(model), np.unique(truth))


@pytest.mark.parametrize("centre, span_r, mrd", [(("-1.543689012692076361570855971", "0"), 1e-25, 3000), (M51, 1e-35, 3000),
                                                 (("-2", "0"), 1e-30, 3000)])
def test_truth_is_stable_in_precision(centre, span_r, mrd):
    """The truth itself does not move between P + 128 and P + 512 fraction bits (the tip included: it is the model that is
    wrong there, not the reference)."""
    orbit, dr, di = _sample(centre, span_r, None, mrd, pixels=60)
    P = orbit.precision_bits
    a = D.direct_counts(centre[0], centre[1], dr, di, mrd, P + 128)
    b = D.direct_counts(centre[0], centre[1], dr, di, mrd, P + 512)
    assert len(np.unique(a)) >= 5 and np.array_equal(a, b)
