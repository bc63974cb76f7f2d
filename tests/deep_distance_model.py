"""The contract of include/mbk.h, "Distance estimates for deep views", in numpy, and its truth -- a helper module, not a
conftest.  Written from the header's text, not from the C code.

    state   zp = fl(Z_1 + dc) (z_0 = c), D = (1, 0), e = 0                                     d = D 2^e
    step    u = fl(fl(zp.r Dr) - fl(zp.i Di)), v = fl(fl(zp.r Di) + fl(zp.i Dr)), D = (fl(2u + one), 2v), one = ldexp(1, -e)
            max(|Dr|, |Di|) >= 2^256: D = fl(D 2^-256), e = min(e + 256, 2^30)                 tested on every step
            then the deep step of deep_model.model_counts, unchanged; zp = the z it tests
    n       the deep count; n > 0: the escaping step's rebase test, then run on until mag >= 2^32 or 64 further steps
    rel     ldexp(fl(fl(fl(sqrt(fl(mag / dmagD))) fl(ln mag)) / f), -(e + k)),  range_r = f 2^k, 0.5 <= f < 1;
            0 if n = 0, 0 instead of NaN

numpy rounds every operation on its own, so the states (n, zp, D, e, mag, dmagD) are the contract's bit for bit; only ln can
separate two implementations of rel (ln_candidates / assert_states_agree, as in distance_model.py).  hp_sample() runs
d' = 2 z d + 1, z' = z^2 + c in mpmath from the exact c = C + dc.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

import deep_model as D

RUN_ON = 64
RADIUS2 = 2.0 ** 32
RESCALE_AT = 2.0 ** 256
RESCALE_BY = 2.0 ** -256
RESCALE_EXP = 256
EXP_CAP = 1 << 30
PRECISION_BITS = 256          # of expression_true

# Relative error of the model's rel (binary64 perturbed orbit and scaled derivative) against the same recurrences in mpmath at
# P + 128 bits from the exact pixel coordinate, on the escaped picks of tests/test_deep_distance.py::CASES whose count and
# run-on length agree (100 picks per case, seed 1; the test prints the figure per case).  Measured: see MEASURED_REL below;
# the worst, one digit rounded up, x 4 because d is an orbit-long product whose error grows with n.
MEASURED_REL = {
    "i-1e-30": 4.7e-14, "i-1e-200": 1.1e-13, "i-1e-280": 8.1e-12, "M51-1e-35": 1.2e-8, "M41-1e-25": 1.9e-11,
    "seahorse-1e-12": 1.1e-8,
}
DEEP_DERIVATIVE_REL = 8e-8    # worst measured 1.2e-8 (M51) -> 2e-8 x 4
# Error of mbk_deep_distance_value_host (glibc's ln; IEEE division, square root, product and the division by f) against the
# correctly rounded expression, in ulps of the truth's nearest double, over the exact (mag, dmagD, e, range_r) of the cases:
# measured by tests/test_deep_distance.py::test_output_rule_against_mpmath, which prints it, fails above DD0 and fails if DD0
# is more than 0.1 above the measurement.  Measured 2.0881 at mag = 1.1187237487469965e+17, dmagD = 2.6615170362676474e+80,
# e = 0, range_r = 1e-30 (c = i): distance_model.D0 (1.95) and part of the half ulp of the division by f.
DD0 = 2.09


def _dstep(zpr, zpi, Dr, Di, e, freeze):
    one = np.ldexp(1.0, (-e).astype(np.int32))
    p0 = zpr * Dr
    p1 = zpi * Di
    p2 = zpr * Di
    p3 = zpi * Dr
    u = p0 - p1
    v = p2 + p3
    Dr = (2.0 * u) + one
    Di = 2.0 * v
    if not freeze:
        big = np.maximum(np.abs(Dr), np.abs(Di)) >= RESCALE_AT
        Dr = np.where(big, Dr * RESCALE_BY, Dr)
        Di = np.where(big, Di * RESCALE_BY, Di)
        e = np.where(big, np.minimum(e + RESCALE_EXP, EXP_CAP), e)
    return Dr, Di, e


def _zstep(T, dr, di, m, cr, ci):
    zr, zi, z2r, z2i = T
    ar = z2r[m] + dr
    ai = z2i[m] + di
    ndr = (ar * dr - ai * di) + cr
    ndi = (ar * di + ai * dr) + ci
    m = m + 1
    xr = zr[m] + ndr
    xi = zi[m] + ndi
    mg = xr * xr + xi * xi
    return ndr, ndi, m, xr, xi, mg


def _rebase(M, ndr, ndi, m, xr, xi, mg):
    reb = (mg < ndr * ndr + ndi * ndi) | (m == M)
    return np.where(reb, xr, ndr), np.where(reb, xi, ndi), np.where(reb, 0, m)


def states(zr, zi, dcr, dci, mrd, *, freeze_e=False):
    """Orbit table (zr, zi) and flat offsets -> dict of flat arrays: n (int32), extra (run-on steps taken), Dr, Di, e, mag at
    the final state, dmagD.  freeze_e: never rescale (e stays 0: the plain contract's binary64 derivative)."""
    zr = np.asarray(zr, np.float64)
    zi = np.asarray(zi, np.float64)
    M = zr.size - 1
    T = (zr, zi, zr + zr, zi + zi)
    cr = np.array(dcr, np.float64).ravel()
    ci = np.array(dci, np.float64).ravel()
    N = cr.size
    n = np.zeros(N, np.int32)
    extra = np.zeros(N, np.int32)
    fin = {k: np.zeros(N, np.float64) for k in ("Dr", "Di", "mag", "dr", "di", "zpr", "zpi")}
    fin["Dr"][:] = 1.0
    fe = np.zeros(N, np.int64)
    fm = np.zeros(N, np.int64)
    with np.errstate(all="ignore"):
        idx = np.arange(N)
        m = np.ones(N, np.int64)
        zpr, zpi = zr[1] + cr, zi[1] + ci
        dr, di = cr.copy(), ci.copy()
        if M == 1:
            dr, di = zpr.copy(), zpi.copy()
            m[:] = 0
        Dr, Di, e = np.ones(N), np.zeros(N), np.zeros(N, np.int64)
        c_r, c_i = cr, ci
        for i in range(1, int(mrd)):
            if idx.size == 0:
                break
            Dr, Di, e = _dstep(zpr, zpi, Dr, Di, e, freeze_e)
            ndr, ndi, m, zpr, zpi, mg = _zstep(T, dr, di, m, c_r, c_i)
            esc = mg >= 4.0
            if esc.any():
                w = idx[esc]
                n[w] = i
                for k, a in (("Dr", Dr), ("Di", Di), ("mag", mg), ("dr", ndr), ("di", ndi), ("zpr", zpr), ("zpi", zpi)):
                    fin[k][w] = a[esc]
                fe[w], fm[w] = e[esc], m[esc]
                keep = ~esc
                idx, c_r, c_i, ndr, ndi, m, zpr, zpi, mg, Dr, Di, e = (a[keep] for a in (idx, c_r, c_i, ndr, ndi, m, zpr, zpi, mg,
                                                                                        Dr, Di, e))
            dr, di, m = _rebase(M, ndr, ndi, m, zpr, zpi, mg)
        # pixels that never escaped keep the state of their last step (their output is 0 whatever it is)
        fin["Dr"][idx], fin["Di"][idx], fe[idx] = Dr, Di, e
        # the run-on of the escaped pixels: first the rebase test the count loop stopped before
        idx = np.flatnonzero(n > 0)
        c_r, c_i = cr[idx], ci[idx]
        Dr, Di, e, mg, zpr, zpi = fin["Dr"][idx], fin["Di"][idx], fe[idx], fin["mag"][idx], fin["zpr"][idx], fin["zpi"][idx]
        dr, di, m = _rebase(M, fin["dr"][idx], fin["di"][idx], fm[idx], zpr, zpi, mg)
        for _ in range(RUN_ON):
            go = ~(mg >= RADIUS2)
            if not go.any():
                break
            nDr, nDi, ne = _dstep(zpr, zpi, Dr, Di, e, freeze_e)
            ndr, ndi, nm, nzr, nzi, nmg = _zstep(T, dr, di, m, c_r, c_i)
            ndr, ndi, nm = _rebase(M, ndr, ndi, nm, nzr, nzi, nmg)
            Dr, Di, e, dr, di, m, zpr, zpi, mg = (np.where(go, a, b) for a, b in (
                (nDr, Dr), (nDi, Di), (ne, e), (ndr, dr), (ndi, di), (nm, m), (nzr, zpr), (nzi, zpi), (nmg, mg)))
            extra[idx[go]] += 1
        fin["Dr"][idx], fin["Di"][idx], fe[idx], fin["mag"][idx] = Dr, Di, e, mg
        out = {"n": n, "extra": extra, "Dr": fin["Dr"], "Di": fin["Di"], "e": fe, "mag": fin["mag"]}
        a = out["Dr"] * out["Dr"]
        b = out["Di"] * out["Di"]
        out["dmagD"] = a + b
    return out


def value(mag, dmagD, e, range_r, n, ln=None):
    """The output expression on arrays; ln: the logarithms to use (default numpy's)."""
    mag = np.asarray(mag, np.float64)
    f, k = math.frexp(float(range_r))
    with np.errstate(all="ignore"):
        q = mag / np.asarray(dmagD, np.float64)
        r = np.sqrt(q)
        l = np.log(mag) if ln is None else ln
        de = r * l
        g = de / np.float64(f)
        rel = np.ldexp(g, (-(np.asarray(e, np.int64) + k)).astype(np.int32))
    rel = np.where(np.isnan(rel), 0.0, rel)
    return np.where(np.asarray(n) > 0, rel, 0.0)


def model(orbit, view, mrd, window=None, **kw):
    """(rel, counts, states) of a DeepView on a DeepOrbit, arrays [nrows, ncols] (states flat)."""
    zr, zi = orbit.table()
    dcr, dci = D.offsets(view, window)
    st = states(zr, zi, dcr, dci, mrd, **kw)
    nrows, ncols = (window[3], window[2]) if window is not None else (view.height, view.width)
    rel = value(st["mag"], st["dmagD"], st["e"], view.span_r, st["n"])
    return rel.reshape(nrows, ncols), st["n"].reshape(nrows, ncols), st


def ln_candidates(st, range_r, reach=2):
    """rel for ln within `reach` ulps of numpy's on either side: [2 reach + 1, N]."""
    with np.errstate(all="ignore"):
        l = np.log(st["mag"])
        outs = []
        for j in range(-reach, reach + 1):
            lj = l.copy()
            for _ in range(abs(j)):
                lj = np.nextafter(lj, np.inf if j > 0 else -np.inf)
            outs.append(value(st["mag"], st["dmagD"], st["e"], range_r, st["n"], ln=lj))
    return np.stack(outs)


def assert_states_agree(got, st, range_r, what):
    """`got` (flat rel of an implementation) is the model's rel bit for bit wherever its ln agrees with numpy's, and elsewhere
    what a neighbouring ln gives.  Returns the share that matches numpy's ln itself."""
    got = np.asarray(got, np.float64).ravel()
    cand = ln_candidates(st, range_r)
    assert not np.isnan(got).any(), what
    hit = (cand == got[None, :]).any(axis=0)
    mid = cand.shape[0] // 2
    assert hit.all(), (what, int((~hit).sum()), [(int(i), int(st["n"][i]), float(st["mag"][i]), float(st["dmagD"][i]), int(st["e"][i]),
                                                  float(got[i]), float(cand[mid, i])) for i in np.flatnonzero(~hit)[:5]])
    return float((cand[mid] == got).mean())


def expression_true(mag, dmagD, range_r):
    """(nearest double, mpf) of g = sqrt(mag / dmagD) ln mag / f on exact, finite, positive doubles: the mantissa of rel."""
    f, _ = math.frexp(float(range_r))
    with mpmath.workprec(PRECISION_BITS):
        v = mpmath.sqrt(mpmath.mpf(float(mag)) / mpmath.mpf(float(dmagD))) * mpmath.log(mpmath.mpf(float(mag))) / mpmath.mpf(f)
        return float(v), v


def hp_sample(centre, dc_r, dc_i, span_r, n_model, extra_model, bits):
    """d' = 2 z d + 1, z' = z^2 + c at `bits` bits from the exact c = C + dc, for the model's count and run-on length:
    (agrees, rel as a float)."""
    Cr, Ci = D.exact(centre[0]) + Fraction(float(dc_r)), D.exact(centre[1]) + Fraction(float(dc_i))
    with mpmath.workprec(bits):
        c = mpmath.mpc(mpmath.mpf(Cr.numerator) / Cr.denominator, mpmath.mpf(Ci.numerator) / Ci.denominator)
        z, d = c, mpmath.mpc(1)
        n = 0
        for k in range(1, int(n_model) + 1):
            d = 2 * z * d + 1
            z = z * z + c
            if z.real * z.real + z.imag * z.imag >= 4:
                n = k
                break
        if n != n_model:
            return False, math.nan
        extra = 0
        while extra < RUN_ON and not (z.real * z.real + z.imag * z.imag >= RADIUS2):
            d = 2 * z * d + 1
            z = z * z + c
            extra += 1
        if extra != extra_model:
            return False, math.nan
        mag = z.real * z.real + z.imag * z.imag
        dmag = d.real * d.real + d.imag * d.imag
        return True, float(mpmath.sqrt(mag / dmag) * mpmath.log(mag) / mpmath.mpf(float(span_r)))
