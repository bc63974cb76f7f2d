// mbk_deep_distance.h -- exterior distance estimates for deep views (include/mbk.h, "Distance estimates for deep views"):
// the deep step of mbk_deep.h with the derivative d = dz/dc riding in it as D 2^e, the run-on to the large radius, and the
// output expression, which the kernel and mbk_deep_distance_value_host share.
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own), per step,
// BEFORE the z step, from zp = the pixel's full z of the previous step (the z = Z_m + dz the deep step computes for its
// bailout test: the loop keeps it, it costs nothing):
//   u = fl(fl(zp.r Dr) - fl(zp.i Di)), v = fl(fl(zp.r Di) + fl(zp.i Dr))
//   Dr = fma(u, 2, one) = fl(2u + one), Di = 2 v          one = 2^-e as a binary64 (subnormal, then 0, past e = 1022)
//   max(|Dr|, |Di|) >= 2^256:  Dr, Di *= 2^-256, e += 256, one = ldexp(1, -e)
// 8 fp64 VALU for the derivative (4 mul, sub, add, fma, the doubling: mbk_distance.h on why the doubling is not folded away)
// and the rescale test on EVERY step, as the contract defines it: one v_max_f64 with |.| source modifiers, one v_cmp, and a
// scalar branch on the wave's ballot over the (rare) rescale block.  |D| < 2^256 before a step and |zp| < 2^16.5 (the run-on's radius) bound every
// product by 2^274: nothing overflows, so no lazy schedule -- and no proof of equal bits -- is needed.
//
// D, e, one and zp do not change at a rebase, so they stay out of the rebase branch: the phi copies of the parent loop
// (profiles/deep/README.md) are not added to.  e is a VGPR (lanes differ).
//
// The main loop has deep_view_kernel's shape (one lane per pixel, 8x8 block per single-wave workgroup, image order, the orbit
// entries from the cursor of mbk_deep_cursor.h).  A lane that escapes leaves it; when the wave is through, the escaped lanes run
// on together in a second, short loop that reads its entries by index (deep_run_on, which mbk_deep_distance_bla.h and the host
// twins call too).
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_deep.h"
#include "mbk_distance.h"

namespace mbk {

constexpr double kDeepRescaleAt = 0x1p256;     // max(|Dr|, |Di|) at or above this is scaled ...
constexpr double kDeepRescaleBy = 0x1p-256;    // ... by this
constexpr int32_t kDeepRescaleExp = 256;
constexpr int32_t kDeepExpCap = 1 << 30;       // e saturates here (rel is 0 long before: the exponent cannot wrap)

// rel = de / range_r with the exponents kept apart: range_r = f 2^k, 0.5 <= f < 1,
//   rel = ldexp(fl(fl(fl(sqrt(fl(mag / dmagD))) fl(ln mag)) / f), -(e + k)),
// 0 for a pixel that never escaped, 0 instead of NaN, dmagD = 0 gives +inf.
__host__ __device__ inline double deep_distance_value(double mag, double dmagD, int32_t e, double range_r, int32_t count)
{
    if (count <= 0) return 0.0;
    int k = 0;
    const double f = frexp(range_r, &k);
    const double q = mag / dmagD;
    const double r = sqrt(q);
    const double l = log(mag);
    const double de = r * l;
    const double g = de / f;
    const double rel = ldexp(g, -(e + k));
    return rel == rel ? rel : 0.0;
}

struct DeepDistanceArgs {
    DeepArgs v;         // orbit, offsets, window, mrd; counts may be null; bytes and smooth are not used
    double range_r;     // the view's real span: the unit of the output
    double *rel;
};

// d' = 2 zp d + 1 on the scaled pair, and the rescale (__host__ too: the host twin of mbk_deep_distance_bla.h calls it)
__host__ __device__ __forceinline__ void deep_derivative_step(double zpr, double zpi, double &Dr, double &Di, int32_t &e, double &one)
{
    const double p0 = zpr * Dr, p1 = zpi * Di, p2 = zpr * Di, p3 = zpi * Dr;
    const double u = p0 - p1;
    const double v = p2 + p3;
    Dr = __builtin_fma(u, 2.0, one);
    Di = 2.0 * v;
    if (__builtin_expect(__builtin_fabs(Dr) >= kDeepRescaleAt || __builtin_fabs(Di) >= kDeepRescaleAt, 0)) {
        Dr *= kDeepRescaleBy;
        Di *= kDeepRescaleBy;
        e = e + kDeepRescaleExp < kDeepExpCap ? e + kDeepRescaleExp : kDeepExpCap;
        one = ldexp(1.0, -e);
    }
}

// the table's entry m as the kernels hold it, from the device's table or from the host's flat one
__host__ __device__ __forceinline__ double4 deep_entry(const double4 *Z, uint32_t m) { return Z[m]; }
__host__ __device__ __forceinline__ double4 deep_entry(const double *Z, uint32_t m)
{
    return make_double4(Z[4 * (size_t)m], Z[4 * (size_t)m + 1], Z[4 * (size_t)m + 2], Z[4 * (size_t)m + 3]);
}

// The run-on of a pixel that escaped with |z|^2 = mag at orbit index m, shared by the kernels and the host twins: the escaping
// step's rebase test (the count loop stopped before it), then plain steps that read their entries by index until mag reaches
// the large radius.  m < M at the top of every step, so entries m and m + 1 exist (entry 0 is (0, 0, 0, 0)).  Returns the
// number of steps taken.
template <typename Table>
__host__ __device__ __forceinline__ int32_t deep_run_on(const Table *Z, uint32_t M, uint32_t m, double dcr, double dci, double &dzr, double &dzi,
                                                        double &zpr, double &zpi, double &mag, double &Dr, double &Di, int32_t &e, double &one)
{
    if (deep_rebase(mag, dzr, dzi) || m == M) {
        dzr = zpr;
        dzi = zpi;
        m = 0u;
    }
    int32_t extra = 0;
    for (; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
        deep_derivative_step(zpr, zpi, Dr, Di, e, one);
        const double4 zm = deep_entry(Z, m), zn = deep_entry(Z, m + 1u);
        deep_plain_step(zm.z, zm.w, dcr, dci, dzr, dzi);
        ++m;
        zpr = zn.x + dzr;
        zpi = zn.y + dzi;
        mag = zpr * zpr + zpi * zpi;
        if (deep_rebase(mag, dzr, dzi) || m == M) {
            dzr = zpr;
            dzi = zpi;
            m = 0u;
        }
    }
    return extra;
}

__global__ __launch_bounds__(64) void deep_distance_kernel(DeepDistanceArgs q)
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
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        deep_derivative_step(zpr, zpi, Dr, Di, e, one);
        deep_plain_step(c.cur.z, c.cur.w, dcr, dci, dzr, dzi);
        c.step();
        zpr = c.nz.x + dzr;
        zpi = c.nz.y + dzi;
        const double mg = zpr * zpr + zpi * zpi;
        if (mg >= 4.0) {
            count = i;
            mag = mg;
            break;
        }
        if (deep_rebase(mg, dzr, dzi) || c.last()) {
            dzr = zpr;
            dzi = zpi;
            c.rebased();
        } else {
            c.advanced();
        }
        c.prefetch();
    }
    if (count > 0) deep_run_on(p.orbit, c.M, c.m, dcr, dci, dzr, dzi, zpr, zpi, mag, Dr, Di, e, one);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = count;
    const double r2 = Dr * Dr, i2 = Di * Di;
    q.rel[o] = deep_distance_value(mag, r2 + i2, e, q.range_r, count);
}

}  // namespace mbk
