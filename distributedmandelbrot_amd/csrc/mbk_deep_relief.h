// mbk_deep_relief.h -- relief shading for deep views (include/mbk.h, "Relief shading for deep views"): the loops of
// deep_distance_kernel (mbk_deep_distance.h) and deep_distance_bla_kernel (mbk_deep_distance_bla.h) with another epilogue.
// Those kernels end every escaped pixel with its full z (zp) and the derivative D 2^e in registers, after the run-on to the
// large radius; the unit normal of z conj(d) does not depend on the scale of d, so e drops out and normal_value (mbk_relief.h)
// takes (zp, D) as it takes (z, d) of a plain view.
//
// One pass, one lane per pixel, 8x8 blocks, the cursors of mbk_deep_cursor.h: a deep sample costs thousands of perturbation
// steps and is paid once.  Per pixel the kernel stores the normal (16 bytes) and, each where the caller wants it, the count,
// nu = smooth_value(n, mag of the ESCAPING step) -- the bits of the count launch's smooth values, which is why that mag is kept
// across the run-on in a register of its own -- and rel = deep_distance_value of the final state, the bits of the distance
// launch.
//
// One templated body serves both kernels: kBla picks the cursor and adds the skip side of the step, everything else -- the
// start, the plain side (deep_derivative_step, deep_plain_step), the bailout / rebase tail, deep_run_on and the epilogue -- is
// written once, from the functions the distance kernels call.  The distance kernels themselves are not touched.  An orbit of
// length 1 has no table and takes the plain kernel, whatever the flag (deep_start's rebased start is the plain cursor's alone).
//
// Magnitudes (include/mbk.h has the full statement): max(|Dr|, |Di|) < 2^256 by both rescale rules and |zp|^2 < 2^65 after the
// run-on -- a step from |z| < 2^16 lands below 2^32 + 2 -- so m = |zp conj(D)|^2 < 2^580: no overflow.  m can underflow to 0,
// which stores the flat normal for an escaped pixel: |zp| >= 2 there, so it takes max(|Dr|, |Di|) < 2^-538.  Nothing forbids
// that: deep_derivative_step rescales downwards only (a step from |zp| < 1/2 shrinks D while e stays), and the upward rescale of
// deep_derivative_skip runs once per skip, by 2^256, and only while e >= 256.  At e < 256 such a D is a true |d| < 2^-282, a
// pixel on a critical point of z_n(c) where the gradient has no direction; the tests assert that no case comes near it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbk_deep_distance_bla.h"
#include "mbk_relief.h"

namespace mbk {

struct DeepReliefArgs {
    DeepBlaArgs b;      // b.v: orbit, offsets, window, mrd; counts and smooth may be null; bytes is not used.  The table: kBla only
    double range_r;     // the view's real span: the unit of rel
    double *normal;     // [n][2]; 8-byte alignment is enough
    double *rel;        // may be null
};

// The cursor of each rule, constructed in place from the kernel's arguments as the distance kernels construct theirs (handed
// back from a function or a lambda the struct is built through a pointer and 64 bytes of it go to scratch).  m0: deep_start's.
template <bool kBla>
struct DeepReliefCursor : OrbitCursor<double4> {
    __device__ __forceinline__ DeepReliefCursor(const DeepBlaArgs &t, uint32_t m0) : OrbitCursor<double4>(t.v.orbit, t.v.z1, t.v.M, m0) {}
};
template <>
struct DeepReliefCursor<true> : BlaCursor<double4, double> {
    // the radius is level 0's rc; 0 at m == 0.  M >= 2: m0 is 1
    __device__ __forceinline__ DeepReliefCursor(const DeepBlaArgs &t, uint32_t) : BlaCursor<double4, double>(t.v.orbit, t.v.z1, t.v.M, t.rc, 0.0) {}
};

template <bool kBla>
__device__ __forceinline__ void deep_relief_body(const DeepReliefArgs &q)
{
    const DeepBlaArgs &t = q.b;
    const DeepArgs &p = t.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const double dcr = px.dcr, dci = px.dci;
    double dzr, dzi, zpr, zpi;           // zp starts as z_0 = c = fl(Z_1 + dc)
    DeepReliefCursor<kBla> c(t, deep_start(p.z1.x, p.z1.y, p.M, dcr, dci, dzr, dzi, zpr, zpi));   // (kBla: M >= 2, m = 1, dz = dc)
    double Dr = 1.0, Di = 0.0, one = 1.0;
    int32_t e = 0;
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        bool skipped = false;
        if constexpr (kBla) {
            double ad;
            if (bla_within(dzr, dzi, c.r0, &ad)) {
                const uint32_t l = bla_climb(t.rc, t.off, t.levels, c.M, c.m, i, p.mrd, ad);
                const double4 ab = t.ab[t.off[l] + ((c.m - 1u) >> l)];
                deep_derivative_skip(ab.x, ab.y, ab.z, ab.w, Dr, Di, e);
                one = ldexp(1.0, -e);
                bla_apply(ab.x, ab.y, ab.z, ab.w, dcr, dci, dzr, dzi);
                c.skip(l);
                i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
                skipped = true;
            }
        }
        if (!skipped) {
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
    const double escaped = mag;          // nu is the count launch's: of the escaping step, before the run-on
    if (count > 0) deep_run_on(p.orbit, c.M, c.m, dcr, dci, dzr, dzi, zpr, zpi, mag, Dr, Di, e, one);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    normal_value(zpr, zpi, Dr, Di, count, q.normal + 2u * o);
    if (p.counts) p.counts[o] = count;
    if (p.smooth) p.smooth[o] = smooth_value(count, escaped);
    if (q.rel) {
        const double r2 = Dr * Dr, i2 = Di * Di;
        q.rel[o] = deep_distance_value(mag, r2 + i2, e, q.range_r, count);
    }
}

__global__ __launch_bounds__(64) void deep_relief_kernel(DeepReliefArgs q) { deep_relief_body<false>(q); }
__global__ __launch_bounds__(64) void deep_relief_bla_kernel(DeepReliefArgs q) { deep_relief_body<true>(q); }

// The host twin of both kernels is deep_distance_bla_host (mbk_deep_distance_bla.h), which hands out the final zp and the
// escaping mag as well: a table without levels gives the plain rule.  normal_value and smooth_value then run on the host.

}  // namespace mbk
