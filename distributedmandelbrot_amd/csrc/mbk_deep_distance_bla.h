// mbk_deep_distance_bla.h -- distance estimates for deep views that take bilinear-approximation skips (include/mbk.h,
// "Distance estimates for deep views with bilinear approximation"): deep_bla_kernel's steps (mbk_deep_bla.h) on the same cursor
// (mbk_deep_cursor.h) with the derivative of mbk_deep_distance.h riding in them, the derivative across a skip, and the one-pixel
// host twin the CPU tests read.
//
// No second table: d is the derivative of the pixel's full z = Z_m + dz with respect to c, and the reference orbit does not
// depend on dc, so across a skip dz -> A dz + B dc the derivative follows d -> A d + B with the coefficients the count table
// already holds.  What is neglected is of the order of the |dz| / |Z| that the radius test bounds by 2^-40 per step.
//
// The skip on d = D 2^e (deep_derivative_skip, shared by the kernel and the host twin): A and B are any finite binary64 (high
// levels reach 1e308) and |D| < 2^256, so the product is formed on mantissas -- As = A 2^-ea, Bs = B 2^-eb with the larger
// component in [0.5, 1) -- and the two terms are aligned to the larger exponent before they are added, as the wide number
// system does (mbk_deep_wide.h).  |As D| < 2^257 per component and |Bs| < 1: nothing overflows, and one 2^256 rescale brings
// the sum back under the plain rule's bound.  The rescale is two-sided: |As| < 1 moves up to a binade per skip from D into e,
// so a sum below 2^-256 is scaled up by 2^256 (while e >= 256) and max(|Dr|, |Di|) stays in [2^-256, 2^256) however long the
// orbit.  e may fall (|A| < 1 where the orbit passes near 0) and is no multiple of 256.
//
// The kernel: the skip side does the level search, loads (A, B) once, runs the derivative skip, then the dz map; the plain side
// is deep_derivative_step and deep_plain_step; the z / bailout / rebase tail is common, and zp is the z it forms (at the new m
// after a skip).  D, e, one and zp stay out of the rebase branch.  The run-on is deep_run_on (mbk_deep_distance.h): plain
// steps only.  After the first rebase the lanes of a wave hold different m: no wave-uniform value is taken from a lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mbk_deep_bla.h"
#include "mbk_deep_distance.h"

namespace mbk {

constexpr int kDeepSkipShiftFloor = -1200;   // an addend that far below the other is dropped (ldexp to 0), never a wrap

// d' = A d + B on d = (Dr, Di) 2^e, and the 2^256 rescale.  The caller recomputes one = ldexp(1, -e).
__host__ __device__ inline void deep_derivative_skip(double Ar, double Ai, double Br, double Bi, double &Dr, double &Di, int32_t &e)
{
    const double aa = __builtin_fabs(Ar), ab = __builtin_fabs(Ai), ba = __builtin_fabs(Br), bb = __builtin_fabs(Bi);
    int ea = 0, eb = 0;
    (void)frexp(aa > ab ? aa : ab, &ea);
    (void)frexp(ba > bb ? ba : bb, &eb);
    const double asr = ldexp(Ar, -ea), asi = ldexp(Ai, -ea);
    const double bsr = ldexp(Br, -eb), bsi = ldexp(Bi, -eb);
    const double p0 = asr * Dr, p1 = asi * Di, p2 = asr * Di, p3 = asi * Dr;
    const double pr = p0 - p1;
    const double pi = p2 + p3;
    const int32_t pe = e + ea;
    int32_t h = pe > eb ? pe : eb;
    if (h < 0) h = 0;
    const int sp = pe - h > kDeepSkipShiftFloor ? pe - h : kDeepSkipShiftFloor;
    const int sb = eb - h > kDeepSkipShiftFloor ? eb - h : kDeepSkipShiftFloor;
    const double xr = ldexp(pr, sp), xi = ldexp(pi, sp);
    const double yr = ldexp(bsr, sb), yi = ldexp(bsi, sb);
    Dr = xr + yr;
    Di = xi + yi;
    if (__builtin_fabs(Dr) >= kDeepRescaleAt || __builtin_fabs(Di) >= kDeepRescaleAt) {
        Dr *= kDeepRescaleBy;
        Di *= kDeepRescaleBy;
        h += kDeepRescaleExp;
    } else if (__builtin_fabs(Dr) < kDeepRescaleBy && __builtin_fabs(Di) < kDeepRescaleBy && h >= kDeepRescaleExp) {
        Dr *= kDeepRescaleAt;   // |As| < 1: every skip may cost D a binade that e gains; without this D decays over a long orbit
        Di *= kDeepRescaleAt;   // (1e-207 after 3000 skips at mrd 30 000) until fl(Dr^2) + fl(Di^2) underflows and rel is inf
        h -= kDeepRescaleExp;
    }
    e = h < kDeepExpCap ? h : kDeepExpCap;
}

struct DeepDistanceBlaArgs {
    DeepBlaArgs b;      // b.v: orbit, offsets, window, mrd; counts may be null; bytes and smooth are not used.  M >= 2
    double range_r;     // the view's real span: the unit of the output
    double *rel;
};

__global__ __launch_bounds__(64) void deep_distance_bla_kernel(DeepDistanceBlaArgs q)
{
    const DeepBlaArgs &t = q.b;
    const DeepArgs &p = t.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const double dcr = px.dcr, dci = px.dci;
    double dzr = dcr, dzi = dci;
    BlaCursor<double4, double> c(p.orbit, p.z1, p.M, t.rc, 0.0);   // the radius is level 0's rc; 0 at m == 0
    double zpr = p.z1.x + dcr, zpi = p.z1.y + dci;     // z_0 = c = fl(Z_1 + dc)
    double Dr = 1.0, Di = 0.0, one = 1.0;
    int32_t e = 0;
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        double ad;
        if (bla_within(dzr, dzi, c.r0, &ad)) {
            const uint32_t l = bla_climb(t.rc, t.off, t.levels, c.M, c.m, i, p.mrd, ad);
            const double4 ab = t.ab[t.off[l] + ((c.m - 1u) >> l)];
            deep_derivative_skip(ab.x, ab.y, ab.z, ab.w, Dr, Di, e);
            one = ldexp(1.0, -e);
            bla_apply(ab.x, ab.y, ab.z, ab.w, dcr, dci, dzr, dzi);
            c.skip(l);
            i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
        } else {
            deep_derivative_step(zpr, zpi, Dr, Di, e, one);
            deep_plain_step(c.cur.z, c.cur.w, dcr, dci, dzr, dzi);
            c.step();
        }
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

// One pixel on the host, from the functions the kernel uses: the count, the run-on steps taken, the final mag (0 for count 0),
// the final D 2^e and the number of steps executed in the count loop (a skip is one).  `orbit` as for build_bla_table; with no
// table (M <= 1, or a table without levels) this is the rule of "Distance estimates for deep views".  For the relief twin
// (mbk_deep_normal_host), each where given: the final zp, and |z|^2 of the escaping step, before the run-on (0 for count 0).
inline void deep_distance_bla_host(const std::vector<double> &orbit, uint32_t M, const BlaTable &t, double dcr, double dci, int64_t mrd,
                                   int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e_out, uint64_t *steps,
                                   double *zp_r = nullptr, double *zp_i = nullptr, double *escaped = nullptr)
{
    const double *Z = orbit.data();
    double dzr, dzi, zpr, zpi;
    uint32_t m = deep_start(Z[4], Z[5], M, dcr, dci, dzr, dzi, zpr, zpi);
    double Dr = 1.0, Di = 0.0, one = 1.0;
    int32_t e = 0;
    *count = 0;
    *extra = 0;
    *mag = 0.0;
    *steps = 0;
    for (int64_t i = 1; i < mrd; ++i) {
        ++*steps;
        double ad;
        if (t.levels && m >= 1u && bla_within(dzr, dzi, t.rc[m - 1u], &ad)) {
            const uint32_t l = bla_climb(t.rc.data(), t.off, t.levels, M, m, i, mrd, ad);
            const double *c = &t.ab[4 * ((size_t)t.off[l] + ((m - 1u) >> l))];
            deep_derivative_skip(c[0], c[1], c[2], c[3], Dr, Di, e);
            one = ldexp(1.0, -e);
            bla_apply(c[0], c[1], c[2], c[3], dcr, dci, dzr, dzi);
            m += 1u << l;
            i += ((int64_t)1 << l) - 1;
        } else {
            deep_derivative_step(zpr, zpi, Dr, Di, e, one);
            deep_plain_step(Z[4 * (size_t)m + 2], Z[4 * (size_t)m + 3], dcr, dci, dzr, dzi);
            ++m;
        }
        zpr = Z[4 * (size_t)m] + dzr;
        zpi = Z[4 * (size_t)m + 1] + dzi;
        const double mg = zpr * zpr + zpi * zpi;
        if (mg >= 4.0) {
            *count = (int32_t)i;
            *mag = mg;
            break;
        }
        if (deep_rebase(mg, dzr, dzi) || m == M) {
            dzr = zpr;
            dzi = zpi;
            m = 0u;
        }
    }
    if (escaped) *escaped = *mag;
    if (*count > 0) *extra = deep_run_on(Z, M, m, dcr, dci, dzr, dzi, zpr, zpi, *mag, Dr, Di, e, one);
    *D_r = Dr;
    *D_i = Di;
    *e_out = e;
    if (zp_r) *zp_r = zpr;
    if (zp_i) *zp_i = zpi;
}

}  // namespace mbk
