// mbk_deep_distance_bla.h -- distance estimates for deep views that take bilinear-approximation skips (include/mbk.h,
// "Distance estimates for deep views with bilinear approximation"): the loop of deep_bla_kernel (mbk_deep_bla.h) with the
// derivative of deep_distance_kernel (mbk_deep_distance.h) riding in it, the derivative across a skip, and the one-pixel host
// twin the CPU tests read.
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
// after a skip).  D, e, one and zp stay out of the rebase branch.  The run-on is deep_distance_kernel's second loop: plain
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
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    if (lc >= p.ncols || lr >= p.nrows) return;
    const double dcr = ((double)(p.col0 + lc) - p.half_r) * p.step_r;
    const double dci = ((double)(p.row0 + lr) - p.half_i) * p.step_i;
    const uint32_t M = p.M, n0 = M - 1u;
    double dzr = dcr, dzi = dci;
    uint32_t m = 1u;
    double c2r = p.z1.z, c2i = p.z1.w;                 // 2 Z_m
    double4 nz = p.orbit[2];                           // entry m + 1 (M >= 2)
    double4 pre = p.orbit[3u < M ? 3u : M];            // entry m + 2 (clamped: unused once m + 1 == M)
    double q0 = t.rc[0];                               // level 0's rc at m (0 at m == 0: the plain step)
    double qn = t.rc[1u < n0 ? 1u : n0 - 1u];          // ... at m + 1 (clamped: unused once m + 1 == M)
    double zpr = p.z1.x + dcr, zpi = p.z1.y + dci;     // z_0 = c = fl(Z_1 + dc)
    double Dr = 1.0, Di = 0.0, one = 1.0;
    int32_t e = 0;
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        double ad;
        if (bla_within(dzr, dzi, q0, &ad)) {
            const uint32_t l = bla_climb(t.rc, t.off, t.levels, M, m, i, p.mrd, ad);
            const double4 c = t.ab[t.off[l] + ((m - 1u) >> l)];
            deep_derivative_skip(c.x, c.y, c.z, c.w, Dr, Di, e);
            one = ldexp(1.0, -e);
            bla_apply(c.x, c.y, c.z, c.w, dcr, dci, dzr, dzi);
            m += 1u << l;                              // <= M: entry j of level l ends at 1 + (j + 1) 2^l <= 1 + (M - 1)
            i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
            nz = p.orbit[m];
            pre = p.orbit[m + 1u < M ? m + 1u : M];
            qn = t.rc[(m < M ? m : n0) - 1u];          // level 0 at the new m (unused at m == M: the rebase)
        } else {
            deep_derivative_step(zpr, zpi, Dr, Di, e, one);
            deep_plain_step(c2r, c2i, dcr, dci, dzr, dzi);
            ++m;
        }
        zpr = nz.x + dzr;
        zpi = nz.y + dzi;
        const double mg = zpr * zpr + zpi * zpi;
        if (mg >= 4.0) {
            count = i;
            mag = mg;
            break;
        }
        const double dm = dzr * dzr + dzi * dzi;
        if (mg < dm || m == M) {   // rebase: the pixel's own z becomes its offset from Z_0 = 0
            dzr = zpr;
            dzi = zpi;
            m = 0u;
            c2r = 0.0;
            c2i = 0.0;
            nz = p.z1;
            q0 = 0.0;
        } else {
            c2r = nz.z;
            c2i = nz.w;
            nz = pre;
            q0 = qn;
        }
        pre = p.orbit[m + 2u < M ? m + 2u : M];
        qn = t.rc[m < n0 ? m : n0 - 1u];
    }
    if (count > 0) {
        // the escaping step's rebase test (the count loop stopped before it), then the run-on, plain steps only: m < M at the top
        // of every step, so entries m and m + 1 exist (entry 0 is (0, 0, 0, 0))
        {
            const double dm = dzr * dzr + dzi * dzi;
            if (mag < dm || m == M) {
                dzr = zpr;
                dzi = zpi;
                m = 0u;
            }
        }
        for (int extra = 0; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
            deep_derivative_step(zpr, zpi, Dr, Di, e, one);
            const double4 zm = p.orbit[m], zn = p.orbit[m + 1u];
            deep_plain_step(zm.z, zm.w, dcr, dci, dzr, dzi);
            ++m;
            zpr = zn.x + dzr;
            zpi = zn.y + dzi;
            mag = zpr * zpr + zpi * zpi;
            const double dm = dzr * dzr + dzi * dzi;
            if (mag < dm || m == M) {
                dzr = zpr;
                dzi = zpi;
                m = 0u;
            }
        }
    }
    const size_t o = (size_t)lr * p.ncols + lc;
    if (p.counts) p.counts[o] = count;
    const double r2 = Dr * Dr, i2 = Di * Di;
    q.rel[o] = deep_distance_value(mag, r2 + i2, e, q.range_r, count);
}

// One pixel on the host, from the functions the kernel uses: the count, the run-on steps taken, the final mag (0 for count 0),
// the final D 2^e and the number of steps executed in the count loop (a skip is one).  `orbit` as for build_bla_table; with no
// table (M <= 1) this is the rule of "Distance estimates for deep views".
inline void deep_distance_bla_host(const std::vector<double> &orbit, uint32_t M, const BlaTable &t, double dcr, double dci, int64_t mrd,
                                   int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e_out, uint64_t *steps)
{
    const double *Z = orbit.data();
    double dzr = dcr, dzi = dci;
    uint32_t m = 1u;
    double zpr = Z[4] + dcr, zpi = Z[5] + dci;
    if (M == 1u) {
        dzr = zpr;
        dzi = zpi;
        m = 0u;
    }
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
        const double dm = dzr * dzr + dzi * dzi;
        const bool rebase = mg < dm || m == M;
        if (rebase) {   // (for an escaping step this is the rebase the run-on starts with)
            dzr = zpr;
            dzi = zpi;
            m = 0u;
        }
        if (mg >= 4.0) {
            *count = (int32_t)i;
            *mag = mg;
            break;
        }
    }
    if (*count > 0)
        for (; *extra < kDistanceRunOn && !(*mag >= kDistanceRadius2); ++*extra) {
            deep_derivative_step(zpr, zpi, Dr, Di, e, one);
            deep_plain_step(Z[4 * (size_t)m + 2], Z[4 * (size_t)m + 3], dcr, dci, dzr, dzi);
            ++m;
            zpr = Z[4 * (size_t)m] + dzr;
            zpi = Z[4 * (size_t)m + 1] + dzi;
            *mag = zpr * zpr + zpi * zpi;
            const double dm = dzr * dzr + dzi * dzi;
            if (*mag < dm || m == M) {
                dzr = zpr;
                dzi = zpi;
                m = 0u;
            }
        }
    *D_r = Dr;
    *D_i = Di;
    *e_out = e;
}

}  // namespace mbk
