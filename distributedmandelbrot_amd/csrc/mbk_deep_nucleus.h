// mbk_deep_nucleus.h -- atom periods and Newton seeds of deep views (include/mbk.h, "Locating minibrots in deep views"): the
// steps of deep_distance_kernel (mbk_deep_distance.h) on the cursor of mbk_deep_cursor.h, with no run-on.  Beside the count each
// pixel keeps the step at which its |z| was smallest and the state there, and stores that step as its atom period and one Newton
// step from the pixel towards the root of z_p(c) = 0.  The host side -- the Newton step and the size estimate at an orbit's own
// centre, in the wide arithmetic of mbk_deep_wide_distance.h -- is below the kernel.
//
// Per step, in deep_distance_kernel's order: deep_derivative_step (d' = 2 zp d + 1 on D 2^e with its 2^256 rescale), the z step,
// mg = |z|^2, the bailout test, then
//     mg < best:  best = mg, arg = i, z_b = zp, (D_b, e_b) = (D, e)          strict: the first minimum wins
// and the rebase tail unchanged.  The escaping z is never a candidate (the bailout test comes first).  The kept values do not
// change at a rebase and are not read inside the loop: they stay out of the rebase branch, as D, e, one and zp do.
//
// The output is delta = -z_b / (D_b 2^e_b) as a fraction of range_r, with the exponents kept apart to the end as
// deep_distance_value does: the quotient is formed on the mantissas and one ldexp applies -(e_b + k).  The translation unit is
// compiled -ffp-contract=off: every operation of deep_nucleus_delta rounds on its own.
//
// One lane per pixel, one 8x8 block per single-wave workgroup, image order (deep_pixel), the orbit entry prefetched a step ahead
// (OrbitCursor); no wave-uniform value is taken from a lane.  deep_nucleus_host runs the same functions on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mbk_deep_bla.h"
#include "mbk_deep_distance.h"
#include "mbk_deep_wide_distance.h"

namespace mbk {

// what a pixel keeps of the step at which its |z|^2 was smallest
struct NucleusBest {
    double best;       // |z_arg|^2
    int32_t arg;       // the step (0: z_0 = c)
    double zr, zi;     // z_arg
    double Dr, Di;     // d_arg = D 2^e
    int32_t e;
};

__host__ __device__ __forceinline__ void deep_nucleus_keep(NucleusBest &b, double mg, int32_t i, double zr, double zi, double Dr, double Di,
                                                           int32_t e)
{
    if (mg < b.best) {
        b.best = mg;
        b.arg = i;
        b.zr = zr;
        b.zi = zi;
        b.Dr = Dr;
        b.Di = Di;
        b.e = e;
    }
}

// delta = -z / (D 2^e) / range_r with range_r = f 2^k, 0.5 <= f < 1:
//   den = fl(fl(Dr^2) + fl(Di^2));  N = (fl(fl(zr Dr) + fl(zi Di)), fl(fl(zi Dr) - fl(zr Di)))        z conj(D)
//   delta = ldexp(-fl(fl(N / den) / f), -(e + k)) per component; a non-finite component makes both +inf ("no seed")
__host__ __device__ inline void deep_nucleus_delta(double zr, double zi, double Dr, double Di, int32_t e, double range_r, double *out_r,
                                                   double *out_i)
{
    int k = 0;
    const double f = frexp(range_r, &k);
    const double r2 = Dr * Dr, i2 = Di * Di;
    const double den = r2 + i2;
    const double a0 = zr * Dr, a1 = zi * Di, b0 = zi * Dr, b1 = zr * Di;
    const double nr = a0 + a1, ni = b0 - b1;
    const double qr = nr / den, qi = ni / den;
    const double gr = qr / f, gi = qi / f;
    double xr = ldexp(-gr, -(e + k)), xi = ldexp(-gi, -(e + k));
    const double inf = __builtin_inf();
    if (!(__builtin_fabs(xr) < inf) || !(__builtin_fabs(xi) < inf)) {
        xr = inf;
        xi = inf;
    }
    *out_r = xr;
    *out_i = xi;
}

struct DeepNucleusArgs {
    DeepArgs v;         // orbit, offsets, window, mrd; counts may be null; bytes and smooth are not used
    double range_r;     // the view's real span: the unit of delta
    int32_t *period;
    double *delta;      // two per pixel: (re, im)
};

__global__ __launch_bounds__(64) void deep_nucleus_kernel(DeepNucleusArgs q)
{
    const DeepArgs &p = q.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const double dcr = px.dcr, dci = px.dci;
    double dzr, dzi, zpr, zpi;           // zp starts as z_0 = c
    OrbitCursor<double4> c(p.orbit, p.z1, p.M, deep_start(p.z1.x, p.z1.y, p.M, dcr, dci, dzr, dzi, zpr, zpi));
    double Dr = 1.0, Di = 0.0, one = 1.0;
    int32_t e = 0;
    int32_t count = 0;
    NucleusBest b = {zpr * zpr + zpi * zpi, 0, zpr, zpi, 1.0, 0.0, 0};
    for (int32_t i = 1; i < p.mrd; ++i) {
        deep_derivative_step(zpr, zpi, Dr, Di, e, one);
        deep_plain_step(c.cur.z, c.cur.w, dcr, dci, dzr, dzi);
        c.step();
        zpr = c.nz.x + dzr;
        zpi = c.nz.y + dzi;
        const double mg = zpr * zpr + zpi * zpi;
        if (mg >= 4.0) {
            count = i;
            break;
        }
        deep_nucleus_keep(b, mg, i, zpr, zpi, Dr, Di, e);
        // one value, not two short-circuited tests: the compiler then selects over the rebase instead of branching around it,
        // which is 7 % faster with the kept state live (profiles/deep_shared/README.md)
        const bool last = c.last();
        if (deep_rebase(mg, dzr, dzi) | last) {
            dzr = zpr;
            dzi = zpi;
            c.rebased();
        } else {
            c.advanced();
        }
        c.prefetch();
    }
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = count;
    q.period[o] = b.arg + 1;
    double xr, xi;
    deep_nucleus_delta(b.zr, b.zi, b.Dr, b.Di, b.e, q.range_r, &xr, &xi);
    q.delta[2u * o] = xr;
    q.delta[2u * o + 1u] = xi;
}

// One pixel on the host, from the functions the kernel uses: the count, the kept state and delta.
inline void deep_nucleus_host(const std::vector<double> &orbit, uint32_t M, double dcr, double dci, double range_r, int64_t mrd,
                              int32_t *count, NucleusBest *best, double *delta)
{
    const double *Z = orbit.data();
    double dzr, dzi, zpr, zpi;
    uint32_t m = deep_start(Z[4], Z[5], M, dcr, dci, dzr, dzi, zpr, zpi);
    double Dr = 1.0, Di = 0.0, one = 1.0;
    int32_t e = 0;
    *count = 0;
    const double s0 = zpr * zpr, s1 = zpi * zpi;
    NucleusBest b = {s0 + s1, 0, zpr, zpi, 1.0, 0.0, 0};
    for (int64_t i = 1; i < mrd; ++i) {
        deep_derivative_step(zpr, zpi, Dr, Di, e, one);
        deep_plain_step(Z[4 * (size_t)m + 2], Z[4 * (size_t)m + 3], dcr, dci, dzr, dzi);
        ++m;
        zpr = Z[4 * (size_t)m] + dzr;
        zpi = Z[4 * (size_t)m + 1] + dzi;
        const double a = zpr * zpr, c = zpi * zpi;
        const double mg = a + c;
        if (mg >= 4.0) {
            *count = (int32_t)i;
            break;
        }
        deep_nucleus_keep(b, mg, (int32_t)i, zpr, zpi, Dr, Di, e);
        if (deep_rebase(mg, dzr, dzi) || m == M) {
            dzr = zpr;
            dzi = zpi;
            m = 0u;
        }
    }
    *best = b;
    deep_nucleus_delta(b.zr, b.zi, b.Dr, b.Di, b.e, range_r, &delta[0], &delta[1]);
}

// ---- the host side: Newton step and size estimate at an orbit's own centre, wide arithmetic ------------------------------

// a wide complex (xr, xi) 2^xe; the zero is (0, 0, kWideZeroExp)
struct WideComplex {
    double r, i;
    int32_t e;
};

inline WideComplex wide_cnorm(double vr, double vi, int32_t e)
{
    WideComplex w;
    wide_norm(vr, vi, e, w.r, w.i, w.e);
    return w;
}

inline WideComplex wide_cmul(const WideComplex &a, const WideComplex &b)
{
    const double p0 = a.r * b.r, p1 = a.i * b.i, p2 = a.r * b.i, p3 = a.i * b.r;
    if ((a.r == 0.0 && a.i == 0.0) || (b.r == 0.0 && b.i == 0.0)) return WideComplex{0.0, 0.0, kWideZeroExp};
    return wide_cnorm(p0 - p1, p2 + p3, a.e + b.e);
}

inline WideComplex wide_cadd(const WideComplex &a, const WideComplex &b)
{
    const int32_t h = wide_max(a.e, b.e);
    return wide_cnorm(wide_sh(a.r, a.e - h) + wide_sh(b.r, b.e - h), wide_sh(a.i, a.e - h) + wide_sh(b.i, b.e - h), h);
}

// 1 / a; a zero a gives a non-finite mantissa
inline WideComplex wide_crcp(const WideComplex &a)
{
    const double r2 = a.r * a.r, i2 = a.i * a.i;
    const double den = r2 + i2;
    return wide_cnorm(a.r / den, -a.i / den, -a.e);
}

// -Z_p / D_p at the orbit's centre: D_1 = 1, D_{k+1} = 2 Z_k D_k + 1 carried by wide_dstep; M >= p >= 1
inline WideComplex wide_newton_step(const std::vector<WideEntry> &Z, uint32_t p)
{
    double Dr = 0.5, Di = 0.0;   // norm((1, 0), 0)
    int32_t e = 1;
    for (uint32_t k = 1; k < p; ++k) wide_dstep(Z[k].xr, Z[k].xi, Z[k].xe, Dr, Di, e);
    const WideComplex z = {-Z[p].xr, -Z[p].xi, Z[p].xe};
    return wide_cmul(z, wide_crcp(WideComplex{Dr, Di, e}));
}

// 1 / (b l^2), l = prod_{k=1}^{p-1} 2 Z_k, b = 1 + sum_{k=1}^{p-1} 1 / l_k over the partial products; M >= p >= 1
inline WideComplex wide_size_estimate(const std::vector<WideEntry> &Z, uint32_t p)
{
    WideComplex l = {0.5, 0.0, 1}, b = {0.5, 0.0, 1};
    for (uint32_t k = 1; k < p; ++k) {
        l = wide_cmul(l, WideComplex{Z[k].xr, Z[k].xi, Z[k].xe + 1});
        b = wide_cadd(b, wide_crcp(l));
    }
    return wide_crcp(wide_cmul(b, wide_cmul(l, l)));
}

}  // namespace mbk
