// mbk_julia.h -- Julia views: z -> z^2 + c with a FIXED parameter c and the pixel as the starting point (include/mbk.h,
// "Julia views"; NOT in the reference, which iterates the Mandelbrot map only).
//
// Contract (tests/julia_model.py restates it in numpy): z_0 = the pixel's coordinate (np.linspace, as every view), never
// tested; z_(k+1) = z_k^2 + c in binary64, every operation rounded on its own in the reference's order; n = the first k >= 1
// with fl(fl(zr^2) + fl(zi^2)) >= 4 (false for NaN), at most mrd - 1 updates, 0 if none.  At a pixel whose coordinate is c the
// orbit is the Mandelbrot orbit of c, so n is calc_mb_value(c).
//
// The kernel is the hand-scheduled loops of mbk_loops.inc seeded with z_0 (escape_count_asm_from / escape_count_group_from):
// one wave per 8x8 block, single-wave workgroups, image order.  What differs from tile_asm_kernel and why it is a kernel of
// its own:
//   * c is a kernel argument, wave-uniform: the two host decisions that tile_asm_kernel takes per wave or per window are taken
//     ONCE per launch here and select the instantiation --
//       literal doubling  fma(2, fl(zr zi), c_i) == fl(fl(fl(2 zr) zi) + c_i) unless zr zi is a non-zero subnormal.  A Julia
//                         orbit's zi is not tied to c_i (with c_i = 0 a row with a tiny z0_i keeps zi tiny for many steps), so
//                         the hazard is not confined to a view's rows: the fma form is taken only when |c_i| >= 2^-900, where
//                         both candidate addends (|2 zr zi| < 2^-1021) are below a quarter ulp of c_i and round away alike.
//                         Every other c_i, 0 included, takes the literal 8-operation loop (MBK_STEP_HEAD_SAFE), per step.
//       grouped test      "|z|^2 >= 4 stays >= 4" holds for |c|^2 < 4 - 1e-9 whatever z is: |z'| >= |z|^2 - |c| > 2 + 2e-10.
//                         For a larger |c| a |z| >= 2 that is below |c| can come back inside, so the whole launch takes the
//                         per-step loop (julia_grouped_ok).
//   * there is no light path: the exterior of a Julia set does not escape within four steps as |c| > 2 does, and the heavy
//     part -- the interior of a connected set, every pixel of it mrd - 1 steps -- is where the grouped loop and the cycle test
//     earn their keep.  The cycle test is exact here for the reason it is there: with c fixed the step is a function of the
//     state's bits alone, and a lane still alive at a check has passed a bailout test since (or, at the first mid-group check
//     of an orbit that started with the grouped loop, compares against its finite z_0, which no state past a |z| >= 2 can equal:
//     |z| grows strictly from there).
// Stores, quantiser and the smooth epilogue are block_pixel's.
#pragma once

#include "mbk_kernels.h"

namespace mbk {

struct JuliaArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;     // 8x8 blocks per block row (1-D grid, image order)
    double cr, ci;         // the parameter
    int32_t mrd;
    uint32_t quant_wide;   // as TileArgs
    double quant_rcp;
    uint32_t exact_steps;  // steps tested one by one before the grouped test takes over
    uint32_t cyc_window;   // MBK_OPT_CYCLE_WINDOW
    int32_t *counts;       // may be null
    uint8_t *bytes;        // may be null
    double *smooth;        // may be null
};

// |c_i| below kSafeImagMin (mbk_kernels.h) takes the literal doubling (see above)
__host__ __device__ inline bool julia_needs_literal(double ci) { return !(__builtin_fabs(ci) >= kSafeImagMin); }

// May a launch with this parameter use the grouped bailout test?  (host arithmetic; the rounding of c2 is 1e-7 of the margin)
inline bool julia_grouped_ok(double cr, double ci) { return cr * cr + ci * ci < 4.0 - 1e-9; }

// The contract's loop for one orbit, in C++: the per-step source the hand-scheduled loops restate (MBK_STEP_HEAD_* /
// MBK_STEP_TAIL, operation for operation), compiled for the host as mbk_julia_count_host.  *mag: |z|^2 of the last step
// executed -- the value that tripped the test for an escaped orbit --, 0 if no step ran.
template <bool kFmaDouble>
__host__ __device__ inline int32_t julia_count(double zr, double zi, double cr, double ci, int32_t mrd, double *mag)
{
    double a = zr * zr, b = zi * zi, m = 0.0;
    int32_t result = 0;
    for (int32_t n = 1; n < mrd; ++n) {
        const double t = a - b;
        double zi_new;
        if (kFmaDouble) {
            const double p = zr * zi;
            zi_new = __builtin_fma(2.0, p, ci);
        } else {
            const double w = zr + zr;
            const double u = w * zi;
            zi_new = u + ci;
        }
        zr = t + cr;
        zi = zi_new;
        a = zr * zr;
        b = zi * zi;
        m = a + b;
        if (m >= 4.0) {
            result = n;
            break;
        }
    }
    *mag = m;
    return result;
}

// kGroup = 0: the per-step loop, every iteration executed (kFmaDouble = false: the literal doubling; it has no grouped form).
// kGroup = 4 / 8 / 16 / 32: kExact steps one by one, then the grouped test; kCycle (8 and 16): with the cycle test.
template <bool kFmaDouble, int kGroup, bool kCycle>
__global__ __launch_bounds__(64) void julia_view_kernel(JuliaArgs p)
{
    static_assert(kFmaDouble || kGroup == 0, "the literal doubling has a per-step loop only");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;   // wave-uniform
    const uint32_t ucol = bx * 8u, urow = by * 8u, lx = lane & 7u, ly = lane >> 3;
    const uint32_t lc = ucol + lx, lr = urow + ly;
    if (lc >= p.ncols || lr >= p.nrows) return;
    const double z0r = axis_value(p.re, p.col0 + lc);
    const double z0i = axis_value(p.im, p.row0 + lr);
    double m = 0;   // |z|^2 at the escaping step (only meaningful when count > 0)
    int32_t count;
    if constexpr (kGroup == 0)
        count = escape_count_asm_from<kFmaDouble>(z0r, z0i, p.cr, p.ci, p.mrd, &m);
    else
        count = escape_count_group_from<kGroup, kCycle>(z0r, z0i, p.cr, p.ci, p.mrd, &m, p.exact_steps, p.cyc_window);
    // (block_pixel: scalar base of the block + a 32-bit lane offset; the window has at most 2^31 pixels)
    const size_t ubase = (size_t)urow * p.ncols + ucol;
    const uint32_t loff = ly * p.ncols + lx;
    if (p.counts) (p.counts + ubase)[loff] = count;
    if (p.bytes) (p.bytes + ubase)[loff] = quantise(count, p.mrd, p.quant_wide, p.quant_rcp);
    if (p.smooth) (p.smooth + ubase)[loff] = smooth_value(count, m);
}

}  // namespace mbk
