// mbk_deep_wide_distance.h -- exterior distance estimates for extended-range deep views (include/mbk.h, "Distance estimates
// for extended-range deep views"): the wide step of mbk_deep_wide.h with the derivative d = dz/dc riding in it as a wide
// complex D 2^e, the run-on of mbk_deep_distance.h to the large radius, and the output expression, which the kernel and
// mbk_deep_xdistance_value_host share.
//
// Per step, BEFORE the z step, from zp = (zv, t), the pixel's full z of the previous step exactly as step (e) left it (nominal
// exponent, not renormalised: the loop holds it anyway):
//   P = (fl(fl(zv_r D_r) - fl(zv_i D_i)), fl(fl(zv_r D_i) + fl(zv_i D_r))), exponent pe = t + e + 1 (the doubling is exact)
//   h = max(pe, 0);  N = (fl(sh(P_r, pe - h) + sh(1, -h)), sh(P_i, pe - h));  (D, e) = norm(N, h), e = min(e, 2^30)
// zp has to be wide: near a deep minibrot the orbit returns to within 1e-400 of 0 while |d| is 1e+400, a binary64 zp is 0
// there and the product is lost -- and for the same reason e may decrease.  Wherever the plain contract of
// mbk_deep_distance.h meets no subnormal, D 2^e is its number (scaling by a power of two is exact) and rel its bits.
//
// D, e and zp do not change at a rebase, so they stay out of the rebase branch, as in mbk_deep_distance.h.  The main loop has
// deep_wide_kernel's shape (one lane per pixel, one 8x8 block per single-wave workgroup in image order, an ordinary divergent
// loop bounded by mrd, the entries from the cursor of mbk_deep_cursor.h, no wave-uniform value taken from a lane).  A lane that
// escapes leaves it; when the wave is through, the escaped lanes run on together in a second, short loop that reads its
// entries by index (wide_run_on, which mbk_deep_wide_distance_bla.h calls too).  wide_distance_host runs the same start, step,
// run-on and value functions on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "mbk_deep_wide.h"
#include "mbk_distance.h"

namespace mbk {

constexpr int32_t kWideDerivativeExpCap = 1 << 30;   // e saturates here (rel is 0 long before: the exponent cannot wrap)

// d' = 2 zp d + 1 on the wide pair: (zr, zi) 2^t is zp, (Dr, Di) 2^e is d
__host__ __device__ inline void wide_dstep(double zr, double zi, int32_t t, double &Dr, double &Di, int32_t &e)
{
    const double p0 = zr * Dr, p1 = zi * Di, p2 = zr * Di, p3 = zi * Dr;
    const double Pr = p0 - p1, Pi = p2 + p3;
    const int32_t pe = t + e + 1, h = wide_max(pe, 0);
    const double Nr = wide_sh(Pr, pe - h) + wide_sh(1.0, -h);
    const double Ni = wide_sh(Pi, pe - h);
    wide_norm(Nr, Ni, h, Dr, Di, e);
    e = e < kWideDerivativeExpCap ? e : kWideDerivativeExpCap;
}

// rel = de / (range_r 2^exp2) with the exponents kept apart: range_r = f 2^k, 0.5 <= f < 1,
//   rel = ldexp(fl(fl(fl(sqrt(fl(mag / dmagD))) fl(ln mag)) / f), -(e + k + exp2)),
// 0 for a pixel that never escaped, 0 instead of NaN, dmagD = 0 gives +inf.
__host__ __device__ inline double wide_distance_value(double mag, double dmagD, int32_t e, double range_r, int32_t exp2, int32_t count)
{
    if (count <= 0) return 0.0;
    const int32_t k = wide_exp(range_r);
    const double f = __builtin_ldexp(range_r, -k);
    const double q = mag / dmagD;
    const double r = sqrt(q);
    const double l = log(mag);
    const double de = r * l;
    const double g = de / f;
    const double rel = __builtin_ldexp(g, -(e + k + exp2));
    return rel == rel ? rel : 0.0;
}

struct DeepWideDistanceArgs {
    DeepWideArgs v;     // orbit, offsets, window, mrd; counts may be null; bytes and smooth are not used
    double range_r;     // the mantissa of the view's real span: with v.exp2 the unit of the output
    double *rel;
};

// The run-on of a pixel that escaped with |z|^2 = mag at orbit index m, shared by the kernels and the host twins: the escaping
// step's rebase test (the count loop stopped before it), then plain steps that read their entries by index until mag reaches
// the large radius.  m < M at the top of every step, so entries m and m + 1 exist (entry 0 is (0, 0, EZ)).  Returns the number
// of steps taken.
__host__ __device__ __forceinline__ int32_t wide_run_on(const WideEntry *Z, uint32_t M, uint32_t m, double dcr, double dci, int32_t exp2, double &wr,
                                                        double &wi, int32_t &q, double &zr, double &zi, int32_t &t, double &mg, double &mag,
                                                        double &Dr, double &Di, int32_t &e)
{
    if (wide_rebase(mg, wr, wi, q, t) || m == M) {
        wide_norm(zr, zi, t, wr, wi, q);
        m = 0u;
    }
    int32_t extra = 0;
    for (; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
        wide_dstep(zr, zi, t, Dr, Di, e);
        const WideEntry zm = Z[m], zn = Z[m + 1u];
        wide_step(zm.xr, zm.xi, zm.xe, dcr, dci, exp2, wr, wi, q);
        ++m;
        wide_z(zn.xr, zn.xi, zn.xe, wr, wi, q, zr, zi, t, mg);
        mag = wide_mag(mg, t);
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
        }
    }
    return extra;
}

__global__ __launch_bounds__(64) void deep_wide_distance_kernel(DeepWideDistanceArgs a)
{
    const DeepWideArgs &p = a.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const double dcr = px.dcr, dci = px.dci;
    const int32_t exp2 = p.exp2;
    double wr, wi, zr, zi, mg;           // zp = (zr, zi) 2^t and its |.|^2 on that exponent; it starts as z_0 = c
    int32_t q, t;
    OrbitCursor<WideEntry> c(p.orbit, p.z1, p.M, wide_start(p.z1, p.M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg));
    double Dr = 0.5, Di = 0.0;           // norm((1, 0), 0)
    int32_t e = 1;
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        wide_dstep(zr, zi, t, Dr, Di, e);
        wide_step(c.cur.xr, c.cur.xi, c.cur.xe, dcr, dci, exp2, wr, wi, q);
        c.step();
        wide_z(c.nz.xr, c.nz.xi, c.nz.xe, wr, wi, q, zr, zi, t, mg);
        const double mgs = wide_mag(mg, t);
        if (mgs >= 4.0) {
            count = i;
            mag = mgs;
            break;
        }
        if (wide_rebase(mg, wr, wi, q, t) || c.last()) {
            wide_norm(zr, zi, t, wr, wi, q);
            c.rebased();
        } else {
            c.advanced();
        }
        c.prefetch();
    }
    if (count > 0) wide_run_on(p.orbit, c.M, c.m, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg, mag, Dr, Di, e);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = count;
    const double r2 = Dr * Dr, i2 = Di * Di;
    a.rel[o] = wide_distance_value(mag, r2 + i2, e, a.range_r, exp2, count);
}

// One pixel on the host, from the functions the kernel uses: the count, the run-on steps taken, the final |z|^2 (0 for count
// 0) and the final derivative D 2^e.
inline void wide_distance_host(const std::vector<WideEntry> &orbit, uint32_t M, double dcr, double dci, int32_t exp2, int64_t mrd,
                               int32_t *count, int32_t *extra, double *mag, double *Dr_out, double *Di_out, int32_t *e_out)
{
    const WideEntry *Z = orbit.data();
    double wr, wi, zr, zi, mg;
    int32_t q, t;
    uint32_t m = wide_start(Z[1], M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg);
    double Dr = 0.5, Di = 0.0;
    int32_t e = 1;
    *count = 0;
    *extra = 0;
    *mag = 0.0;
    for (int64_t i = 1; i < mrd; ++i) {
        wide_dstep(zr, zi, t, Dr, Di, e);
        wide_step(Z[m].xr, Z[m].xi, Z[m].xe, dcr, dci, exp2, wr, wi, q);
        ++m;
        wide_z(Z[m].xr, Z[m].xi, Z[m].xe, wr, wi, q, zr, zi, t, mg);
        const double mgs = wide_mag(mg, t);
        if (mgs >= 4.0) {
            *count = (int32_t)i;
            *mag = mgs;
            break;
        }
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
        }
    }
    if (*count > 0) *extra = wide_run_on(Z, M, m, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg, *mag, Dr, Di, e);
    *Dr_out = Dr;
    *Di_out = Di;
    *e_out = e;
}

}  // namespace mbk
