// mbk_deep_wide_distance_bla.h -- distance estimates for extended-range deep views that take bilinear-approximation skips
// (include/mbk.h, "Distance estimates for extended-range deep views with bilinear approximation"): the loop of
// deep_wide_bla_kernel (mbk_deep_wide_bla.h) with the derivative of deep_wide_distance_kernel (mbk_deep_wide_distance.h) riding
// in it, the derivative across a skip, and the one-pixel host twin the CPU tests read.
//
// No second table: d is the derivative of the pixel's full z = Z_m + dz with respect to c, and the reference orbit does not
// depend on dc, so across a skip dz -> A dz + B dc the derivative follows d -> A d + B with the (A, e_A), (B, e_B) the count
// table already holds.  What is neglected is of the order of the |dz| / |Z| that the radius test bounds by 2^-40 per step.
//
// The skip on d = D 2^e (wide_dskip, shared by the kernel and the host twin) is wide_bla_apply's sum with D in place of w and
// 1 in place of dcm: mantissa products, the two terms aligned to the larger exponent, one norm.  The wide number system needs
// no 2^256 rescale and no floor at 0; e may fall (|A| < 1 where the orbit passes near 0).
//
// The kernel: the skip side does the level search, loads (A, B) once, runs the derivative skip, then the dz map; the plain side
// is wide_dstep and wide_step; the z / bailout / rebase tail is common, and zp is the (zv, t) it forms (at the new m after a
// skip).  D, e and zp stay out of the rebase branch.  The run-on is wide_run_on's loop (mbk_deep_wide_distance.h): plain steps,
// entries read by index.  After the first rebase the lanes of a wave hold different m: no wave-uniform value is taken from a
// lane.  The launch bound asks for 8 waves per SIMD: left to itself the allocator takes 66 VGPRs (7 waves), with the bound 54,
// with no scratch either way.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mbk_deep_wide_bla.h"
#include "mbk_deep_wide_distance.h"

namespace mbk {

// d' = A d + B on the wide pair: (ar, ai) 2^ae is A, (br, bi) 2^be is B, (Dr, Di) 2^e is d
__host__ __device__ inline void wide_dskip(double ar, double ai, int32_t ae, double br, double bi, int32_t be, double &Dr, double &Di,
                                           int32_t &e)
{
    const double p0 = ar * Dr, p1 = ai * Di, p2 = ar * Di, p3 = ai * Dr;
    const double Pr = p0 - p1, Pi = p2 + p3;
    const int32_t pe = ae + e, h = wide_max(pe, be);   // (a zero D or B sits at kWideZeroExp: it never sets h against a live term)
    const double Nr = wide_sh(Pr, pe - h) + wide_sh(br, be - h);
    const double Ni = wide_sh(Pi, pe - h) + wide_sh(bi, be - h);
    wide_norm(Nr, Ni, h, Dr, Di, e);
    e = e < kWideDerivativeExpCap ? e : kWideDerivativeExpCap;
}

struct DeepWideDistanceBlaArgs {
    DeepWideBlaArgs b;  // b.v: orbit, offsets, window, mrd; counts may be null; bytes and smooth are not used.  M >= 2
    double range_r;     // the mantissa of the view's real span: with b.v.exp2 the unit of the output
    double *rel;
};

// This kernel keeps its loop written out -- its own pixel set-up, cursor and run-on, the text deep_wide_bla_kernel and
// deep_wide_distance_kernel had before they moved onto mbk_deep_cursor.h and wide_run_on.  On the shared pieces it compiled to a
// loop that was a steady 0.3 to 0.5 % slower on the seahorse view (profiles/deep_shared/README.md); written out, its ISA is the
// earlier one, instruction for instruction.  A fix to a clamp or to the M == 1 rule has to be made here as well.
__global__ __launch_bounds__(64, 8) void deep_wide_distance_bla_kernel(DeepWideDistanceBlaArgs a)
{
    const DeepWideBlaArgs &b = a.b;
    const DeepWideArgs &p = b.v;
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    if (lc >= p.ncols || lr >= p.nrows) return;
    const double dcr = ((double)(p.col0 + lc) - p.half_r) * p.step_r;
    const double dci = ((double)(p.row0 + lr) - p.half_i) * p.step_i;
    const uint32_t M = p.M, n0 = M - 1u;
    const int32_t exp2 = p.exp2;
    const WideEntry zero = {0.0, 0.0, kWideZeroExp, {0, 0, 0}};
    double wr, wi;
    int32_t q;
    wide_norm(dcr, dci, exp2, wr, wi, q);
    uint32_t m = 1u;
    WideEntry cur = p.z1;                                // entry m
    WideEntry nz = p.orbit[2];                           // entry m + 1 (M >= 2)
    WideEntry pre = p.orbit[3u < M ? 3u : M];            // entry m + 2 (clamped: unused once m + 1 == M)
    int32_t k0 = b.ke[0];                                // level 0's ke at m (kWideZeroExp at m == 0: the plain step)
    int32_t kn = b.ke[1u < n0 ? 1u : n0 - 1u];           // ... at m + 1 (clamped: unused once m + 1 == M)
    double zr, zi, mg;                                   // zp = (zr, zi) 2^t and its |.|^2 on that exponent
    int32_t t;
    wide_z(cur.xr, cur.xi, cur.xe, wr, wi, q, zr, zi, t, mg);   // z_0 = c = Z_1 + dc
    double Dr = 0.5, Di = 0.0;                           // norm((1, 0), 0)
    int32_t e = 1;
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        if (wide_bla_within(q, k0)) {
            uint32_t l;
            const uint32_t at = wide_bla_climb(b.ke, b.off, b.levels, M, m, i, p.mrd, q, &l);
            const WideBlaEntry c = b.ab[at];
            wide_dskip(c.ar, c.ai, c.ae, c.br, c.bi, c.be, Dr, Di, e);
            wide_bla_apply(c.ar, c.ai, c.ae, c.br, c.bi, c.be, dcr, dci, exp2, wr, wi, q);
            m += 1u << l;                              // <= M: entry j of level l ends at 1 + (j + 1) 2^l <= 1 + (M - 1)
            i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
            nz = p.orbit[m];
            pre = p.orbit[m + 1u < M ? m + 1u : M];
            kn = b.ke[(m < M ? m : n0) - 1u];          // level 0 at the new m (unused at m == M: the rebase)
        } else {
            wide_dstep(zr, zi, t, Dr, Di, e);
            wide_step(cur.xr, cur.xi, cur.xe, dcr, dci, exp2, wr, wi, q);
            ++m;
        }
        wide_z(nz.xr, nz.xi, nz.xe, wr, wi, q, zr, zi, t, mg);
        const double mgs = wide_mag(mg, t);
        if (mgs >= 4.0) {
            count = i;
            mag = mgs;
            break;
        }
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {   // rebase: the pixel's own z becomes its offset from Z_0 = 0
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
            cur = zero;
            nz = p.z1;
            k0 = kWideZeroExp;
        } else {
            cur = nz;
            nz = pre;
            k0 = kn;
        }
        pre = p.orbit[m + 2u < M ? m + 2u : M];
        kn = b.ke[m < n0 ? m : n0 - 1u];
    }
    if (count > 0) {
        // the escaping step's rebase test (the count loop stopped before it), then the run-on, plain steps only: m < M at the top
        // of every step, so entries m and m + 1 exist (entry 0 is (0, 0, EZ))
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
        }
        for (int extra = 0; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
            wide_dstep(zr, zi, t, Dr, Di, e);
            const WideEntry zm = p.orbit[m], zn = p.orbit[m + 1u];
            wide_step(zm.xr, zm.xi, zm.xe, dcr, dci, exp2, wr, wi, q);
            ++m;
            wide_z(zn.xr, zn.xi, zn.xe, wr, wi, q, zr, zi, t, mg);
            mag = wide_mag(mg, t);
            if (wide_rebase(mg, wr, wi, q, t) || m == M) {
                wide_norm(zr, zi, t, wr, wi, q);
                m = 0u;
            }
        }
    }
    const size_t o = (size_t)lr * p.ncols + lc;
    if (p.counts) p.counts[o] = count;
    const double r2 = Dr * Dr, i2 = Di * Di;
    a.rel[o] = wide_distance_value(mag, r2 + i2, e, a.range_r, exp2, count);
}

// One pixel on the host, from the functions the kernel uses: the count, the run-on steps taken, the final |z|^2 (0 for count
// 0), the final derivative D 2^e and the number of steps executed in the count loop (a skip is one).  With no table (M <= 1,
// or a table without levels) this is the rule of "Distance estimates for extended-range deep views".  For the relief twin
// (mbk_deep_xview_normal_host), each where given: the final zp = (zr, zi) 2^t, and |z|^2 of the escaping step, before the
// run-on (0 for count 0).
inline void wide_distance_bla_host(const std::vector<WideEntry> &orbit, uint32_t M, const WideBlaTable &tb, double dcr, double dci,
                                   int32_t exp2, int64_t mrd, int32_t *count, int32_t *extra, double *mag, double *Dr_out,
                                   double *Di_out, int32_t *e_out, uint64_t *steps, double *zr_out = nullptr, double *zi_out = nullptr,
                                   int32_t *t_out = nullptr, double *escaped = nullptr)
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
    *steps = 0;
    for (int64_t i = 1; i < mrd; ++i) {
        ++*steps;
        if (tb.levels && m >= 1u && wide_bla_within(q, tb.ke[m - 1u])) {
            uint32_t l;
            const uint32_t at = wide_bla_climb(tb.ke.data(), tb.off, tb.levels, M, m, i, mrd, q, &l);
            const WideBlaEntry &c = tb.ab[at];
            wide_dskip(c.ar, c.ai, c.ae, c.br, c.bi, c.be, Dr, Di, e);
            wide_bla_apply(c.ar, c.ai, c.ae, c.br, c.bi, c.be, dcr, dci, exp2, wr, wi, q);
            m += 1u << l;
            i += ((int64_t)1 << l) - 1;
        } else {
            wide_dstep(zr, zi, t, Dr, Di, e);
            wide_step(Z[m].xr, Z[m].xi, Z[m].xe, dcr, dci, exp2, wr, wi, q);
            ++m;
        }
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
    if (escaped) *escaped = *mag;
    if (*count > 0) *extra = wide_run_on(Z, M, m, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg, *mag, Dr, Di, e);
    *Dr_out = Dr;
    *Di_out = Di;
    *e_out = e;
    if (zr_out) *zr_out = zr;
    if (zi_out) *zi_out = zi;
    if (t_out) *t_out = t;
}

}  // namespace mbk
