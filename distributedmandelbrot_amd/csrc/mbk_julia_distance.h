// mbk_julia_distance.h -- exterior distance estimates for Julia views (include/mbk.h, "Distance estimates for Julia views"):
// the derivative d = dz_k/dz_0 -- with respect to the STARTING POINT, the parameter is fixed -- carried beside the orbit of
// mbk_julia.h, the run-on of mbk_distance.h to the large radius, and that file's output expression (distance_value, shared).
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own):
//   u = fl(fl(zr dr) - fl(zi di)), v = fl(fl(zr di) + fl(zi dr))          from z_k and d_k
//   dr' = 2 u, di' = 2 v                                                  exact in binary64, subnormals included; an overflow
//                                                                          is the infinity IEEE gives.  There is no "+ 1": the
//                                                                          derivative of z^2 + c in z_0 is 2 z d, and d_0 = 1.
//   z' by the recurrence of mbk_julia.h (julia_count), squares shared between |z|^2 and the next update.
// Per step: z 6 fp64 VALU (3 mul, sub, add, fma; 7 with the literal doubling) and d 8 (4 mul, sub, add, the two doublings):
// 14 without the bailout test (distance_step's count: its fma(u, 2, 1) is a doubling here), 16 with it.  The doublings are NOT
// folded into a later operand, for the reason mbk_distance.h gives: fl(zi (2 e)) = 2 fl(zi e) holds only while neither product is
// subnormal, and an output modifier (mul:2) flushes denormals on gfx950.
//
// The parameter is a kernel argument, wave-uniform, so the doubling of zi' is decided on the host once per launch, by the rule
// of the count launch with the same c (julia_needs_literal): the z of both kernels is then the same bits, step for step.
//
// Two forms, both one lane per pixel, 8x8 blocks, single-wave workgroups, image order (distance_kernel's shape):
//   two passes (kOnePass = false)  the counts come from julia_view_kernel (launched first, unchanged: grouped test and cycle
//        test as its own rules decide); a lane runs exactly its n steps with no bailout test -- the step counter is wave-uniform,
//        bounded by the wave's largest n, and a lane leaves by an integer compare against its own n.  A block whose counts are
//        all 0 (the whole interior of a connected set) stores zeros after one load and ends.
//   one pass (kOnePass = true)     the derivative rides in a per-step escape loop; no counts are read, and the counts it writes
//        are the count launch's because z is the same recurrence.
// The run-on does not test `>= 4` again: for |c| > 2 mag may fall below 4 during it, which changes neither n nor the steps.
// A z_0 that is exactly 0 has d_1 = 2 z_0 d_0 = 0 and so d_k = 0 for every k >= 1: with n > 0 its dmag is 0 and it stores +inf
// (distance_value: dmag = 0).  Plain views have no such pixel (their d gains 1 every step).
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_distance.h"
#include "mbk_julia.h"

namespace mbk {

struct JuliaDistanceArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;          // 8x8 blocks per block row (1-D grid, image order)
    double cr, ci;              // the parameter
    int32_t mrd;
    const int32_t *counts_in;   // two passes: julia_view_kernel's counts (window layout)
    int32_t *counts_out;        // one pass: may be null
    double *distance;
};

// One step of both recurrences.  (a, b) = (zr^2, zi^2) come in from the previous step and go out for the next one.
template <bool kFmaDouble>
__host__ __device__ __forceinline__ void julia_distance_step(double &zr, double &zi, double &a, double &b, double &dr, double &di,
                                                             double cr, double ci)
{
    const double p0 = zr * dr, p1 = zi * di, p2 = zr * di, p3 = zi * dr;
    const double u = p0 - p1;
    const double v = p2 + p3;
    const double t = a - b;
    double zi_new;
    if (kFmaDouble) {
        const double p = zr * zi;
        zi_new = __builtin_fma(2.0, p, ci);
    } else {
        const double w = zr + zr;
        const double q = w * zi;
        zi_new = q + ci;
    }
    dr = 2.0 * u;
    di = 2.0 * v;
    zr = t + cr;
    zi = zi_new;
    a = zr * zr;
    b = zi * zi;
}

// One orbit, the contract's loops in the kernel's order: the count loop (at most mrd - 1 updates), then the run-on.  The host
// twin (mbk_julia_distance_host) is this function; the one-pass kernel restates its two loops around the same step.
template <bool kFmaDouble>
__host__ __device__ inline void julia_distance_orbit(double &zr, double &zi, double &dr, double &di, double cr, double ci, int32_t mrd,
                                                     int32_t &n, int32_t &extra, double &mag)
{
    double a = zr * zr, b = zi * zi;
    dr = 1.0;
    di = 0.0;
    n = 0;
    extra = 0;
    for (int32_t k = 1; k < mrd; ++k) {
        julia_distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
        if (a + b >= 4.0) {
            n = k;
            break;
        }
    }
    mag = a + b;
    if (n > 0) {
        for (; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
            julia_distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
            mag = a + b;
        }
    }
}

template <bool kFmaDouble, bool kOnePass>
__global__ __launch_bounds__(64) void julia_distance_kernel(const JuliaDistanceArgs p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    const bool live = lc < p.ncols && lr < p.nrows;
    const size_t o = live ? (size_t)lr * p.ncols + lc : 0u;
    int32_t n = 0;
    if (!kOnePass) {
        if (live) n = p.counts_in[o];
        if (__ballot(n > 0) == 0ull) {   // nothing escaped here: the interior, and the blocks outside the window
            if (live) p.distance[o] = 0.0;
            return;
        }
    }
    const double cr = p.cr, ci = p.ci;   // wave-uniform
    double zr = axis_value(p.re, p.col0 + (live ? lc : 0u));
    double zi = axis_value(p.im, p.row0 + (live ? lr : 0u));
    double dr = 1.0, di = 0.0;
    double a = zr * zr, b = zi * zi;
    if (kOnePass) {
        if (live) {
            for (int32_t k = 1; k < p.mrd; ++k) {
                julia_distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
                if (a + b >= 4.0) {
                    n = k;
                    break;
                }
            }
        }
    } else {
        int32_t nmax = n;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int32_t other = __shfl_xor(nmax, off);
            nmax = other > nmax ? other : nmax;
        }
        nmax = __builtin_amdgcn_readfirstlane(nmax);
        for (int32_t k = 0; k < nmax; ++k)
            if (k < n) julia_distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
    }
    double mag = a + b;
    if (n > 0) {
        for (int extra = 0; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
            julia_distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
            mag = a + b;
        }
    }
    if (!live) return;
    const double r2 = dr * dr, i2 = di * di;
    p.distance[o] = distance_value(mag, r2 + i2, n);
    if (kOnePass && p.counts_out) p.counts_out[o] = n;
}

}   // namespace mbk
