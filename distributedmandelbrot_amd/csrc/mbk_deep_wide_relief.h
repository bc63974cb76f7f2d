// mbk_deep_wide_relief.h -- relief shading for extended-range deep views (include/mbk.h, "Relief shading for extended-range
// deep views"): the loops of deep_wide_distance_kernel (mbk_deep_wide_distance.h) and deep_wide_distance_bla_kernel
// (mbk_deep_wide_distance_bla.h) with another epilogue.  Those kernels end every escaped pixel with its full z = (zr, zi) 2^t
// and the derivative d = (Dr, Di) 2^e in registers, after the run-on to the large radius; the unit normal of z conj(d) depends
// on neither t nor e, so normal_value (mbk_relief.h) takes the four mantissas as it takes (z, d) of a plain view.
//
// One pass, one lane per pixel, 8x8 blocks, the cursors of mbk_deep_cursor.h: a wide sample costs thousands of wide steps and
// is paid once.  Per pixel the kernel stores the normal (16 bytes) and, each where the caller wants it, the count,
// nu = smooth_value(n, mag of the ESCAPING step) -- the bits of the count launch's smooth values, which is why that mag is kept
// across the run-on in a register of its own -- and rel = wide_distance_value of the final state, the bits of the distance
// launch.  After the first rebase the lanes of a wave hold different m: no wave-uniform value is taken from a lane.
//
// One templated body serves both kernels, as deep_relief_body does (mbk_deep_relief.h): kXbla picks the cursor and adds the
// skip side of the step (wide_bla_within, wide_bla_climb, wide_dskip, wide_bla_apply); the start (wide_start), the plain side
// (wide_dstep, wide_step), the z / bailout / rebase tail, wide_run_on and the epilogue are written once, from the functions
// the distance kernels call.  deep_wide_distance_bla_kernel keeps its loop written out because on the cursor it compiled to a
// loop 0.3 to 0.5 % slower; the xbla relief kernel stays on the shared body all the same: there is no earlier instruction
// stream of its own to preserve, a second written-out copy of the loop would be a third place to mend a clamp or the M == 1
// rule, and the measured kernel times (profiles/deep_wide_relief/README.md) say what the choice costs against that kernel.
// The distance kernels themselves are not touched.  An orbit of length 1 has no table and takes the plain kernel, whatever
// the flag (wide_start's rebased start is the plain cursor's alone).
//
// Magnitudes (include/mbk.h has the full statement).  For an escaped pixel the final state is that of a wide_z: t = max(xe, q),
// zr and zi each the sum of two aligned mantissas below 1 in magnitude, so |zr|, |zi| < 2; D is normalised, its larger
// component in [0.5, 1), unless it is exactly 0.  So |wr|, |wi| < 4 and m = |z conj(D)|^2 < 2^5: no overflow.  From below:
// |z| >= 2 (1 - 2^-50) at the escape and does not shrink in the run-on, which ends below |z| = 2^32 + 3 (a step from
// |z| < 2^16 with |c| < 3); the orbit has |Z_m| < 6, so xe <= 3, and |dz| <= |z| + |Z_m| < 2^33 gives q <= 33: t <= 33 and
// |(zr, zi)|^2 = |z|^2 2^-2t > 2^-65, |D|^2 >= 1/4, m > 2^-68 with every rounding counted.  m can neither overflow nor
// underflow: an escaped pixel has the flat normal only where D is exactly 0 (2 z d = -1 to the last bit on the step before),
// and the 2^-538 caveat of mbk_deep_relief.h has no counterpart here.  The tests assert that no escaped pixel of any case is
// flat.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbk_deep_wide_distance_bla.h"
#include "mbk_relief.h"

namespace mbk {

struct DeepWideReliefArgs {
    DeepWideBlaArgs b;  // b.v: orbit, offsets, window, mrd; counts and smooth may be null; bytes is not used.  The table: kXbla only
    double range_r;     // the mantissa of the view's real span: with b.v.exp2 the unit of rel
    double *normal;     // [n][2]; 8-byte alignment is enough
    double *rel;        // may be null
};

// The cursor of each rule, constructed in place from the kernel's arguments as the distance kernels construct theirs.  m0:
// wide_start's.
template <bool kXbla>
struct WideReliefCursor : OrbitCursor<WideEntry> {
    __device__ __forceinline__ WideReliefCursor(const DeepWideBlaArgs &b, uint32_t m0) : OrbitCursor<WideEntry>(b.v.orbit, b.v.z1, b.v.M, m0) {}
};
template <>
struct WideReliefCursor<true> : BlaCursor<WideEntry, int32_t> {
    // the radius is level 0's ke; kWideZeroExp at m == 0.  M >= 2: m0 is 1
    __device__ __forceinline__ WideReliefCursor(const DeepWideBlaArgs &b, uint32_t)
        : BlaCursor<WideEntry, int32_t>(b.v.orbit, b.v.z1, b.v.M, b.ke, kWideZeroExp) {}
};

template <bool kXbla>
__device__ __forceinline__ void deep_wide_relief_body(const DeepWideReliefArgs &a)
{
    const DeepWideBlaArgs &b = a.b;
    const DeepWideArgs &p = b.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const double dcr = px.dcr, dci = px.dci;
    const int32_t exp2 = p.exp2;
    double wr, wi, zr, zi, mg;           // zp = (zr, zi) 2^t and its |.|^2 on that exponent; it starts as z_0 = c
    int32_t q, t;
    WideReliefCursor<kXbla> c(b, wide_start(p.z1, p.M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg));   // (kXbla: M >= 2, m = 1, dz = norm(dc))
    double Dr = 0.5, Di = 0.0;           // norm((1, 0), 0)
    int32_t e = 1;
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        bool skipped = false;
        if constexpr (kXbla) {
            if (wide_bla_within(q, c.r0)) {
                uint32_t l;
                const uint32_t at = wide_bla_climb(b.ke, b.off, b.levels, c.M, c.m, i, p.mrd, q, &l);
                const WideBlaEntry s = b.ab[at];
                wide_dskip(s.ar, s.ai, s.ae, s.br, s.bi, s.be, Dr, Di, e);
                wide_bla_apply(s.ar, s.ai, s.ae, s.br, s.bi, s.be, dcr, dci, exp2, wr, wi, q);
                c.skip(l);
                i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
                skipped = true;
            }
        }
        if (!skipped) {
            wide_dstep(zr, zi, t, Dr, Di, e);
            wide_step(c.cur.xr, c.cur.xi, c.cur.xe, dcr, dci, exp2, wr, wi, q);
            c.step();
        }
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
    const double escaped = mag;          // nu is the count launch's: of the escaping step, before the run-on
    if (count > 0) wide_run_on(p.orbit, c.M, c.m, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg, mag, Dr, Di, e);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    normal_value(zr, zi, Dr, Di, count, a.normal + 2u * o);
    if (p.counts) p.counts[o] = count;
    if (p.smooth) p.smooth[o] = smooth_value(count, escaped);
    if (a.rel) {
        const double r2 = Dr * Dr, i2 = Di * Di;
        a.rel[o] = wide_distance_value(mag, r2 + i2, e, a.range_r, exp2, count);
    }
}

__global__ __launch_bounds__(64) void deep_wide_relief_kernel(DeepWideReliefArgs a) { deep_wide_relief_body<false>(a); }
// (the bound of deep_wide_distance_bla_kernel: 8 waves per SIMD; profiles/deep_wide_relief/README.md has the registers)
__global__ __launch_bounds__(64, 8) void deep_wide_relief_xbla_kernel(DeepWideReliefArgs a) { deep_wide_relief_body<true>(a); }

// The host twin of both kernels is wide_distance_bla_host (mbk_deep_wide_distance_bla.h), which hands out the final zp and the
// escaping mag as well: a table without levels gives the plain rule.  normal_value and smooth_value then run on the host.

}  // namespace mbk
