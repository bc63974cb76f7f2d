// mbk_relief.h -- relief shading for plain views (include/mbk.h, "Relief shading"): the unit normal of the exterior potential's
// height field, taken from the state the distance estimates already carry (mbk_distance.h: the derivative d = dz/dc beside the
// orbit and the run-on to the large radius).  z / d points along the gradient of the potential; z conj(d) has the same
// direction and needs no division before the normalisation.  The epilogue (normal_value) and the shade of a sample
// (relief_shade) are __host__ __device__ functions that the kernels and the host twins share.
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own):
//   wr = fl(fl(zr dr) + fl(zi di)), wi = fl(fl(zi dr) - fl(zr di)), m = fl(fl(wr^2) + fl(wi^2))
//   n = (fl(wr / s), fl(wi / s)), s = fl(sqrt(m)); the flat normal (0, 0) unless 0 < m < inf, and where the count is 0
// Division and square root are the correctly rounded ones and no logarithm is involved: device, host and a numpy restatement
// agree on every bit.
//
// The kernel is distance_kernel's loop (the same two forms, the same steps through distance_step, so the same final state)
// with this epilogue: 16 bytes per pixel for the normal and, when the caller wants them, the 8 of distance_value from the
// same state -- the bits mbk_view_launch_distance stores.
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_distance.h"

namespace mbk {

// out = the unit normal at the final state of a pixel with count > 0; (0, 0) for count 0 and wherever |z conj(d)|^2 is not a
// positive finite number (a NaN or an infinity in the state, underflow to 0, overflow).  Never a NaN.
__host__ __device__ inline void normal_value(double zr, double zi, double dr, double di, int32_t count, double out[2])
{
    const double p0 = zr * dr, p1 = zi * di, p2 = zi * dr, p3 = zr * di;
    const double wr = p0 + p1;
    const double wi = p2 - p3;
    const double r2 = wr * wr, i2 = wi * wi;
    const double m = r2 + i2;
    const bool flat = count <= 0 || !(m > 0.0) || m == INFINITY;
    const double s = sqrt(m);
    const double nx = wr / s, ny = wi / s;
    out[0] = flat ? 0.0 : nx;
    out[1] = flat ? 0.0 : ny;
}

// The brightness q in [0, 256] of a sample with normal (nx, ny) under the light (lx, ly) at height h:
// t = fl(fl(fl(fl(nx lx) + fl(ny ly)) + h) / fl(1 + h)); 0 unless t > 0, 256 from t >= 1 up, floor(256 t) between (exact).
__host__ __device__ inline uint32_t relief_shade(double nx, double ny, double lx, double ly, double h)
{
    const double a = nx * lx, b = ny * ly;
    const double g = a + b;
    const double num = g + h;
    const double den = 1.0 + h;
    const double t = num / den;
    if (!(t > 0.0)) return 0u;
    if (t >= 1.0) return 256u;
    return (uint32_t)(t * 256.0);
}

struct ReliefArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;          // 8x8 blocks per block row (1-D grid, row-major)
    int32_t mrd;
    const int32_t *counts_in;   // two passes: the escape kernels' counts (window layout)
    int32_t *counts_out;        // one pass: may be null
    double *normal;             // [n][2]; 8-byte alignment is enough
    double *distance;           // may be null
};

template <bool kFmaDouble, bool kOnePass>
__global__ __launch_bounds__(64) void relief_kernel(const ReliefArgs p)
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
            if (live) {
                p.normal[2u * o] = 0.0;
                p.normal[2u * o + 1u] = 0.0;
                if (p.distance) p.distance[o] = 0.0;
            }
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
    normal_value(zr, zi, dr, di, n, p.normal + 2u * o);
    if (p.distance) {
        const double r2 = dr * dr, i2 = di * di;
        p.distance[o] = distance_value(mag, r2 + i2, n);
    }
    if (kOnePass && p.counts_out) p.counts_out[o] = n;
}

}   // namespace mbk
