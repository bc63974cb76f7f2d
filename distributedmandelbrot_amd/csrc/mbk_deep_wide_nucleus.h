// mbk_deep_wide_nucleus.h -- atom periods and Newton seeds of extended-range deep views (include/mbk.h, "Locating minibrots in
// extended-range deep views"): the steps of deep_wide_distance_kernel (mbk_deep_wide_distance.h) on the cursor of
// mbk_deep_cursor.h, with no run-on, keeping the minimum as deep_nucleus_kernel (mbk_deep_nucleus.h) does.  Beside the count
// each pixel keeps the step at which its |z| was smallest and the state there, and stores that step as its atom period and one
// Newton step from the pixel towards the root of z_p(c) = 0.
//
// The magnitude that orders the candidates has to be wide: near a deep minibrot |z| is 1e-400 and |z|^2 as a binary64
// (wide_mag) is 0.  From the mg and t that wide_z leaves, |z|^2 = mg 2^(2t) with mg not normalised,
//     nmag(mg, t) = (bm, be):  s = wide_exp(mg), bm = ldexp(mg, -s) in [0.5, 1), be = 2t + s;  mg == 0: (0, -2^30)
//     (bm', be') < (bm, be)  iff  be' < be, or be' == be and bm' < bm
// Per step, in deep_wide_distance_kernel's order: wide_dstep, wide_step, wide_z, mgs = wide_mag(mg, t), the bailout test, then
//     nmag(mg, t) < best:  best = nmag, arg = i, z_b = (zr, zi, t), (D_b, e_b) = (D, e)          strict: the first minimum wins
// and the rebase tail unchanged.  The escaping z is never a candidate (the bailout test comes first).  The exponents are
// compared first: a candidate with the larger be is dropped on the frexp exponent alone, and only a tie or a win pays the ldexp
// that normalises the mantissa -- the bits are the contract's either way.  The kept values do not change at a rebase and are
// not read inside the loop: they stay out of the rebase branch, as D, e and zp do.
//
// The output is delta = -z_b / (D_b 2^e_b) as a fraction of range_r 2^exp2, with the exponents kept apart to the end: the
// quotient is formed on the mantissas exactly as deep_nucleus_delta forms it and one ldexp applies t_b - e_b - k - exp2.  The
// translation unit is compiled -ffp-contract=off: every operation rounds on its own.
//
// One lane per pixel, one 8x8 block per single-wave workgroup, image order, the orbit entry prefetched a step ahead; no
// wave-uniform value is taken from a lane.  62 VGPRs, no scratch; 124 VALU a step where the exponent decides, as the distance
// kernel's loop (profiles/deep_wide_nucleus/README.md).  wide_nucleus_host runs the same functions on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mbk_deep_wide.h"
#include "mbk_deep_wide_distance.h"

namespace mbk {

constexpr int32_t kWideNmagZeroExp = -(1 << 30);   // be of nmag(0, t)

// what a pixel keeps of the step at which its |z|^2 was smallest
struct WideNucleusBest {
    double bm;         // nmag of |z_arg|^2: the mantissa, in [0.5, 1) (0 for a zero z)
    int32_t be;        // and its exponent
    int32_t arg;       // the step (0: z_0 = c)
    double zr, zi;     // z_arg = (zr, zi) 2^t as wide_z left it (not renormalised)
    int32_t t;
    double Dr, Di;     // d_arg = D 2^e
    int32_t e;
};

// nmag(mg, t)
__host__ __device__ inline void wide_nmag(double mg, int32_t t, double &bm, int32_t &be)
{
    if (mg == 0.0) {
        bm = 0.0;
        be = kWideNmagZeroExp;
        return;
    }
    const int32_t s = wide_exp(mg);
    bm = __builtin_ldexp(mg, -s);
    be = 2 * t + s;
}

__host__ __device__ __forceinline__ void wide_nucleus_keep(WideNucleusBest &b, double mg, int32_t i, double zr, double zi, int32_t t, double Dr,
                                                           double Di, int32_t e)
{
    const bool nz = mg != 0.0;
    const int32_t s = nz ? wide_exp(mg) : 0;
    const int32_t be = nz ? 2 * t + s : kWideNmagZeroExp;
    if (be > b.be) return;                        // (decided by the exponent: nothing is normalised)
    const double bm = __builtin_ldexp(mg, -s);    // a tie or a win (a zero mg stays 0)
    if (be == b.be && !(bm < b.bm)) return;
    b.bm = bm;
    b.be = be;
    b.arg = i;
    b.zr = zr;
    b.zi = zi;
    b.t = t;
    b.Dr = Dr;
    b.Di = Di;
    b.e = e;
}

// delta = -z / (D 2^e) / (range_r 2^exp2) with z = (zr, zi) 2^t and range_r = f 2^k, 0.5 <= f < 1: den, N and the two divisions
// of deep_nucleus_delta on the mantissas,
//   delta = ldexp(-fl(fl(N / den) / f), t - e - k - exp2) per component; a non-finite component makes both +inf ("no seed")
__host__ __device__ inline void wide_nucleus_delta(double zr, double zi, int32_t t, double Dr, double Di, int32_t e, double range_r,
                                                   int32_t exp2, double *out_r, double *out_i)
{
    const int32_t k = wide_exp(range_r);
    const double f = __builtin_ldexp(range_r, -k);
    const double r2 = Dr * Dr, i2 = Di * Di;
    const double den = r2 + i2;
    const double a0 = zr * Dr, a1 = zi * Di, b0 = zi * Dr, b1 = zr * Di;
    const double nr = a0 + a1, ni = b0 - b1;
    const double qr = nr / den, qi = ni / den;
    const double gr = qr / f, gi = qi / f;
    const int32_t sh = t - e - k - exp2;   // |t| <= 2^24 + 2^11, -2^11 < e <= 2^30, |k + exp2| < 2^14: no wrap
    double xr = __builtin_ldexp(-gr, sh), xi = __builtin_ldexp(-gi, sh);
    const double inf = __builtin_inf();
    if (!(__builtin_fabs(xr) < inf) || !(__builtin_fabs(xi) < inf)) {
        xr = inf;
        xi = inf;
    }
    *out_r = xr;
    *out_i = xi;
}

struct DeepWideNucleusArgs {
    DeepWideArgs v;     // orbit, offsets, window, mrd; counts may be null; bytes and smooth are not used
    double range_r;     // the mantissa of the view's real span: with v.exp2 the unit of delta
    int32_t *period;
    double *delta;      // two per pixel: (re, im)
};

// the kept state of step 0: z_0 = c = (zr, zi) 2^t with its mg, d_0 = 1
__host__ __device__ __forceinline__ WideNucleusBest wide_nucleus_first(double zr, double zi, int32_t t, double mg)
{
    WideNucleusBest b;
    wide_nmag(mg, t, b.bm, b.be);
    b.arg = 0;
    b.zr = zr;
    b.zi = zi;
    b.t = t;
    b.Dr = 0.5;
    b.Di = 0.0;
    b.e = 1;
    return b;
}

__global__ __launch_bounds__(64) void deep_wide_nucleus_kernel(DeepWideNucleusArgs a)
{
    const DeepWideArgs &p = a.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const double dcr = px.dcr, dci = px.dci;
    const int32_t exp2 = p.exp2;
    double wr, wi, zr, zi, mg;           // zp = (zr, zi) 2^t and its |.|^2 on that exponent; it starts as z_0 = c
    int32_t q, t;
    OrbitCursor<WideEntry> c(p.orbit, p.z1, p.M, wide_start(p.z1, p.M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg));
    WideNucleusBest b = wide_nucleus_first(zr, zi, t, mg);
    double Dr = 0.5, Di = 0.0;           // norm((1, 0), 0)
    int32_t e = 1;
    int32_t count = 0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        wide_dstep(zr, zi, t, Dr, Di, e);
        wide_step(c.cur.xr, c.cur.xi, c.cur.xe, dcr, dci, exp2, wr, wi, q);
        c.step();
        wide_z(c.nz.xr, c.nz.xi, c.nz.xe, wr, wi, q, zr, zi, t, mg);
        const double mgs = wide_mag(mg, t);
        if (mgs >= 4.0) {
            count = i;
            break;
        }
        wide_nucleus_keep(b, mg, i, zr, zi, t, Dr, Di, e);
        if (wide_rebase(mg, wr, wi, q, t) || c.last()) {
            wide_norm(zr, zi, t, wr, wi, q);
            c.rebased();
        } else {
            c.advanced();
        }
        c.prefetch();
    }
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = count;
    a.period[o] = b.arg + 1;
    double xr, xi;
    wide_nucleus_delta(b.zr, b.zi, b.t, b.Dr, b.Di, b.e, a.range_r, exp2, &xr, &xi);
    a.delta[2u * o] = xr;
    a.delta[2u * o + 1u] = xi;
}

// One pixel on the host, from the functions the kernel uses: the count, the kept state and delta.
inline void wide_nucleus_host(const std::vector<WideEntry> &orbit, uint32_t M, double dcr, double dci, double range_r, int32_t exp2,
                              int64_t mrd, int32_t *count, WideNucleusBest *best, double *delta)
{
    const WideEntry *Z = orbit.data();
    double wr, wi, zr, zi, mg;
    int32_t q, t;
    uint32_t m = wide_start(Z[1], M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg);
    WideNucleusBest b = wide_nucleus_first(zr, zi, t, mg);
    double Dr = 0.5, Di = 0.0;
    int32_t e = 1;
    *count = 0;
    for (int64_t i = 1; i < mrd; ++i) {
        wide_dstep(zr, zi, t, Dr, Di, e);
        wide_step(Z[m].xr, Z[m].xi, Z[m].xe, dcr, dci, exp2, wr, wi, q);
        ++m;
        wide_z(Z[m].xr, Z[m].xi, Z[m].xe, wr, wi, q, zr, zi, t, mg);
        if (wide_mag(mg, t) >= 4.0) {
            *count = (int32_t)i;
            break;
        }
        wide_nucleus_keep(b, mg, (int32_t)i, zr, zi, t, Dr, Di, e);
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
        }
    }
    *best = b;
    wide_nucleus_delta(b.zr, b.zi, b.t, b.Dr, b.Di, b.e, range_r, exp2, &delta[0], &delta[1]);
}

}  // namespace mbk
