// mbk_distance.h -- exterior distance estimates for plain views (include/mbk.h, "Distance estimates"): the derivative
// d = dz/dc carried beside the orbit, the run-on to the large radius, and the output expression, which the kernel and
// mbk_distance_value_host share.
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own):
//   u = fl(fl(zr dr) - fl(zi di)), v = fl(fl(zr di) + fl(zi dr))          from z_k and d_k
//   dr' = fma(u, 2, 1) = fl(2u + 1), di' = 2 v                            2u and 2v are exact in binary64, subnormals
//                                                                          included; where 2u overflows, fl(2u + 1) and
//                                                                          fl(fl(2u) + 1) are the same infinity
//   z' by the recurrence of mbk_kernels.h (escape_count), squares shared between |z|^2 and the next update.
// Per step: z 6 fp64 VALU (3 mul, sub, add, fma; 7 with the literal doubling), d 8 (4 mul, sub, add, fma, the doubling),
// and |z|^2 + compare where the bailout is tested: 14 without the test, 16 with it.  The doubling of v is NOT folded into a
// later operand: fl(zi (2 e)) = 2 fl(zi e) holds only while neither product is subnormal, and an output modifier (mul:2)
// flushes denormals on gfx950 -- the eighth slot buys exactness everywhere.
//
// Two forms, both one lane per pixel, 8x8 blocks, single-wave workgroups:
//   two passes (kOnePass = false)  the counts come from the escape kernels (launched first, unchanged); a lane runs exactly
//        its n steps with no bailout test -- the step counter is wave-uniform (an SGPR, bounded by the wave's largest n) and
//        a lane leaves by an integer compare against its own n.  A block whose counts are all 0 (the interior, the bulk of
//        the iterations of any view that holds part of the set) ends after one load.
//   one pass (kOnePass = true)     the derivative rides in a per-step escape loop (`>= 4` tested every step, as kernel "asm"
//        does): no counts are read; the counts it writes are the parity counts because z is the same recurrence.
// The loops are compiler-scheduled from this source (the ISA of the two-pass main loop: 14 v_*_f64, one v_cmp_gt_i32 and
// the scalar loop control per step).
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_kernels.h"

namespace mbk {

constexpr int kDistanceRunOn = 64;        // uncounted steps past the escape, at most
constexpr double kDistanceRadius2 = 0x1p32;   // ... or until |z|^2 reaches this

// de = fl(fl(sqrt(fl(mag / dmag))) * fl(ln mag)) = 2 |z| ln |z| / |d|; 0 for a pixel that never escaped, 0 instead of NaN
// (mag = dmag = inf; a NaN in d), infinities as IEEE gives them (mag = inf: +inf; dmag = inf: 0; dmag = 0: +inf).
__host__ __device__ inline double distance_value(double mag, double dmag, int32_t count)
{
    if (count <= 0) return 0.0;
    const double q = mag / dmag;
    const double r = sqrt(q);
    const double l = log(mag);
    const double de = r * l;
    return de == de ? de : 0.0;
}

struct DistanceArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;          // 8x8 blocks per block row (1-D grid, row-major)
    int32_t mrd;
    const int32_t *counts_in;   // two passes: the escape kernels' counts (window layout)
    int32_t *counts_out;        // one pass: may be null
    double *distance;
};

// One step of both recurrences.  (a, b) = (zr^2, zi^2) come in from the previous step and go out for the next one.
template <bool kFmaDouble>
__device__ __forceinline__ void distance_step(double &zr, double &zi, double &a, double &b, double &dr, double &di, double cr,
                                              double ci)
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
        const double w = 2.0 * zr;
        const double q = w * zi;
        zi_new = q + ci;
    }
    dr = __builtin_fma(u, 2.0, 1.0);
    di = 2.0 * v;
    zr = t + cr;
    zi = zi_new;
    a = zr * zr;
    b = zi * zi;
}

template <bool kFmaDouble, bool kOnePass>
__global__ __launch_bounds__(64) void distance_kernel(const DistanceArgs p)
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
    const double cr = axis_value(p.re, p.col0 + (live ? lc : 0u));
    const double ci = axis_value(p.im, p.row0 + (live ? lr : 0u));
    double zr = cr, zi = ci, dr = 1.0, di = 0.0;
    double a = zr * zr, b = zi * zi;
    if (kOnePass) {
        if (live) {
            for (int32_t k = 1; k < p.mrd; ++k) {
                distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
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
            if (k < n) distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
    }
    double mag = a + b;
    if (n > 0) {
        for (int extra = 0; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
            distance_step<kFmaDouble>(zr, zi, a, b, dr, di, cr, ci);
            mag = a + b;
        }
    }
    if (!live) return;
    const double r2 = dr * dr, i2 = di * di;
    p.distance[o] = distance_value(mag, r2 + i2, n);
    if (kOnePass && p.counts_out) p.counts_out[o] = n;
}

}   // namespace mbk
