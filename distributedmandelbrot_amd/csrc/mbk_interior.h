// mbk_interior.h -- interior views for plain views (include/mbk.h, "Interior views"): for a pixel that never escapes, the period
// of the attracting cycle its orbit settles on and the interior distance estimate from the cycle's derivatives.  The four stages
// of the contract -- cycle (Brent's search for a bitwise repeat), period (the repeat reduced with the 2^-40 tolerance),
// derivatives, output -- are written once as __host__ __device__ functions that the kernel and mbk_interior_host share.
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own):
//   step      z' by the recurrence of mbk_kernels.h (escape_count), the squares (a, b) = (zr^2, zi^2) carried from step to step:
//             6 fp64 VALU with the fused doubling, 7 with the literal one (rows with a tiny c_i, as for every plain-view kernel).
//   cmul      (fl(fl(ar br) - fl(ai bi)), fl(fl(ar bi) + fl(ai br))): 4 mul, sub, add.
//   doublings multiplications by 2, exact; the one rounded doubling is B's real part, fl(2u + 1) = fma(u, 2, 1), as in mbk_distance.h.
//   output    division and square root are the correctly rounded ones; there is no libm call, so host and device agree to the bit.
//
// The kernel is the second of two passes, one lane per pixel, 8x8 blocks, single-wave workgroups like distance_kernel.  The counts
// come from the escape kernels (launched first, unchanged).  A block with no count-0 pixel ends after its one load.  A count-0
// pixel cannot escape within mrd - 1 steps, so the search loop has no bailout test and cannot see a NaN.  The Brent schedule
// (step counter, since, w) is the same for every pixel: inside the loop the three are wave-uniform and live in SGPRs, and the
// reference update is guarded by a scalar compare.  A lane leaves on its hit; the wave ends when no lane is left or after mrd - 1
// steps.  The period and derivative loops run at most L and p steps per lane, after the search: their registers (16 more
// binary64 values) are not live across it.
// The ISA of the search loop as compiled (profiles/interior/README.md): 6 v_*_f64, two v_cmp_ne_u64 and the scalar loop control.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_kernels.h"

namespace mbk {

constexpr double kInteriorTolerance = 0x1p-40;   // the period rule's tolerance: part of the contract

struct InteriorArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;          // 8x8 blocks per block row (1-D grid, row-major)
    int32_t mrd;
    const int32_t *counts_in;   // the escape kernels' counts (window layout)
    int32_t *period;            // may be null
    double *distance;           // may be null
};

__host__ __device__ inline uint64_t interior_bits(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof(u));
    return u;
}

// One step of z; (a, b) = (zr^2, zi^2) come in from the previous step and go out for the next one.
template <bool kFmaDouble>
__host__ __device__ inline void interior_step(double &zr, double &zi, double &a, double &b, double cr, double ci)
{
    const double t = a - b;
    double zi_new;
    if (kFmaDouble) {
        const double p = zr * zi;
        zi_new = __builtin_fma(2.0, p, ci);
    } else {
        const double w = 2.0 * zr;
        const double q = w * zi;
        zi_new = q + ci;
    }
    zr = t + cr;
    zi = zi_new;
    a = zr * zr;
    b = zi * zi;
}

struct Cplx { double r, i; };

__host__ __device__ inline Cplx interior_cmul(Cplx x, Cplx y)
{
    const double p0 = x.r * y.r, p1 = x.i * y.i, p2 = x.r * y.i, p3 = x.i * y.r;
    return Cplx{p0 - p1, p2 + p3};
}

// cycle: Brent's search from z_0 = c for a pixel whose count is 0.  Returns L, the minimal bitwise period, and the reference
// (rr, ri), which lies on the cycle; 0 when no repeat shows within the mrd - 1 updates (unknown).  The hit is tested before the
// reference moves; k, since and w do not depend on the pixel.
template <bool kFmaDouble>
__host__ __device__ inline int32_t interior_cycle(double cr, double ci, int32_t mrd, double &rr, double &ri)
{
    double zr = cr, zi = ci, a = zr * zr, b = zi * zi;
    rr = zr;
    ri = zi;
    uint32_t w = 1u, since = 0u;
    for (int32_t k = 1; k < mrd; ++k) {
        interior_step<kFmaDouble>(zr, zi, a, b, cr, ci);
        ++since;
        if (interior_bits(zr) == interior_bits(rr) && interior_bits(zi) == interior_bits(ri)) return (int32_t)since;
        if (since == w) {
            rr = zr;
            ri = zi;
            w *= 2u;
            since = 0u;
        }
    }
    return 0;
}

// period: the first d in 1 .. L at which the orbit from r is back within the tolerance of r, in both components.  d = L
// qualifies (the orbit is back bit for bit), so the loop needs no other bound.
template <bool kFmaDouble>
__host__ __device__ inline int32_t interior_period(double rr, double ri, double cr, double ci, int32_t L)
{
    double yr = rr, yi = ri, a = yr * yr, b = yi * yi;
    for (int32_t d = 1; d < L; ++d) {
        interior_step<kFmaDouble>(yr, yi, a, b, cr, ci);
        const double er = __builtin_fabs(yr - rr), ei = __builtin_fabs(yi - ri);
        if ((er > ei ? er : ei) <= kInteriorTolerance) return d;
    }
    return L;
}

// derivatives and output: p steps from z = r carrying A = dz, B = dc, E = dzz, F = dcz of the p-fold map, every update from the
// old values; then de = (1 - |A|^2) / |F + E B / (1 - A)|, 0 unless |A|^2 < 1, 0 instead of NaN, +inf for a zero denominator.
template <bool kFmaDouble>
__host__ __device__ inline double interior_distance(double rr, double ri, double cr, double ci, int32_t p)
{
    Cplx z = {rr, ri}, A = {1.0, 0.0}, B = {0.0, 0.0}, E = {0.0, 0.0}, F = {0.0, 0.0};
    double a = z.r * z.r, b = z.i * z.i;
    for (int32_t k = 0; k < p; ++k) {
        const Cplx zF = interior_cmul(z, F), AB = interior_cmul(A, B), AA = interior_cmul(A, A), zE = interior_cmul(z, E);
        const Cplx zB = interior_cmul(z, B), zA = interior_cmul(z, A);
        F = Cplx{2.0 * (zF.r + AB.r), 2.0 * (zF.i + AB.i)};
        E = Cplx{2.0 * (AA.r + zE.r), 2.0 * (AA.i + zE.i)};
        B = Cplx{__builtin_fma(zB.r, 2.0, 1.0), 2.0 * zB.i};
        A = Cplx{2.0 * zA.r, 2.0 * zA.i};
        interior_step<kFmaDouble>(z.r, z.i, a, b, cr, ci);
    }
    const double ar2 = A.r * A.r, ai2 = A.i * A.i;
    const double m2 = ar2 + ai2;
    if (!(m2 < 1.0)) return 0.0;
    const Cplx g = {1.0 - A.r, -A.i};
    const Cplx h = interior_cmul(E, B);
    const Cplx t = interior_cmul(h, Cplx{g.r, -g.i});
    const double gr2 = g.r * g.r, gi2 = g.i * g.i;
    const double gm = gr2 + gi2;
    const double qr = t.r / gm, qi = t.i / gm;
    const double Gr = F.r + qr, Gi = F.i + qi;
    const double Gr2 = Gr * Gr, Gi2 = Gi * Gi;
    const double den = Gr2 + Gi2;
    const double num = 1.0 - m2;
    const double de = num / sqrt(den);
    return de == de ? de : 0.0;
}

// The contract for one pixel given its count (stages 2 to 5): what the kernel's lanes and mbk_interior_host run.
template <bool kFmaDouble>
__host__ __device__ inline void interior_pixel(double cr, double ci, int32_t mrd, int32_t count, int32_t &cycle_len, int32_t &period,
                                               double &de)
{
    cycle_len = 0;
    period = 0;
    de = 0.0;
    if (count != 0) return;
    double rr, ri;
    cycle_len = interior_cycle<kFmaDouble>(cr, ci, mrd, rr, ri);
    if (cycle_len == 0) return;
    period = interior_period<kFmaDouble>(rr, ri, cr, ci, cycle_len);
    de = interior_distance<kFmaDouble>(rr, ri, cr, ci, period);
}

template <bool kFmaDouble>
__global__ __launch_bounds__(64) void interior_kernel(const InteriorArgs p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    const bool live = lc < p.ncols && lr < p.nrows;
    const size_t o = live ? (size_t)lr * p.ncols + lc : 0u;
    const int32_t n = live ? p.counts_in[o] : 1;   // (a lane outside the window takes no part)
    int32_t cycle_len = 0, period = 0;
    double de = 0.0;
    if (__ballot(n == 0) != 0ull) {   // otherwise nothing here lies in the set: the exterior, and the blocks past the window
        const double cr = axis_value(p.re, p.col0 + (live ? lc : 0u));
        const double ci = axis_value(p.im, p.row0 + (live ? lr : 0u));
        interior_pixel<kFmaDouble>(cr, ci, p.mrd, n, cycle_len, period, de);
    }
    if (!live) return;
    if (p.period) p.period[o] = period;
    if (p.distance) p.distance[o] = de;
}

}   // namespace mbk
