// mbk_deep.h -- device side of the deep-zoom views (include/mbk.h, "Deep-zoom views"): perturbation with rebasing.
//
// Each lane iterates its pixel's offset dz from a reference orbit Z_m of the view's centre (mbk_deep_orbit.h) in strict
// binary64 -- every operation rounded on its own, the translation unit is compiled -ffp-contract=off:
//     ar = 2Z_m.r + dz.r ;  ai = 2Z_m.i + dz.i
//     dz = ((ar dz.r - ai dz.i) + dc.r, (ar dz.i + ai dz.r) + dc.i) ;  m = m + 1
//     z = Z_m + dz ;  |z|^2 >= 4 -> count ;  |z|^2 < |dz|^2 or m == M -> dz = z, m = 0
// The table stores (Z, 2Z) per entry (2Z = Z + Z is exact): 32 bytes, two 16-byte loads per lane.
//
// One lane per pixel, one 8x8 block per single-wave workgroup, image order.  The loop is an ordinary divergent loop: a
// lane that escapes leaves EXEC, and the wave leaves when no lane is left (the exec mask -- the ballot of live lanes --
// is empty).  No wave-uniform value is taken from a lane.  Before the first rebase every lane reads the same entry (one
// broadcast line); after that each lane has its own m.  The entry the NEXT step needs, Z_{m+1}, is loaded one step ahead
// (`pre`), so its L1/L2 latency hides behind a step's ~20 dependent fp64 operations; entry 1 (the state right after a
// rebase) comes with the arguments.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbk {

struct DeepArgs {
    const double4 *orbit;     // entries 0 .. M: (Zr, Zi, 2 Zr, 2 Zi)
    double4 z1;               // entry 1
    uint32_t M;               // the orbit's length (>= 1)
    double half_r, half_i;    // (W - 1) / 2, (H - 1) / 2: exact
    double step_r, step_i;    // fl(R / (W - 1)), fl(R_i / (H - 1)); 0 for a single column / row
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;        // 8x8 blocks per row of blocks
    int32_t mrd;
    uint32_t quant_wide;      // the quantiser of mbk_kernels.h (quantise)
    double quant_rcp;
    int32_t *counts;          // may be null
    uint8_t *bytes;           // may be null
    double *smooth;           // may be null
};

__global__ __launch_bounds__(64) void deep_view_kernel(DeepArgs p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    if (lc >= p.ncols || lr >= p.nrows) return;
    // dc = fl(fl(k - (W-1)/2) * s): the subtraction is exact (|k| < 2^32, a half-integer at most)
    const double dcr = ((double)(p.col0 + lc) - p.half_r) * p.step_r;
    const double dci = ((double)(p.row0 + lr) - p.half_i) * p.step_i;
    const uint32_t M = p.M;
    double dzr = dcr, dzi = dci;
    uint32_t m = 1u;
    double c2r = p.z1.z, c2i = p.z1.w;   // 2 Z_m
    double4 nz;                          // entry m + 1
    if (M == 1u) {
        // no Z_2: the start state is rebased at once (z = Z_1 + dc, m = 0)
        dzr = p.z1.x + dcr;
        dzi = p.z1.y + dci;
        m = 0u;
        c2r = 0.0;
        c2i = 0.0;
        nz = p.z1;
    } else {
        nz = p.orbit[2];
    }
    double4 pre = p.orbit[m + 2u < M ? m + 2u : M];   // entry m + 2 (clamped: unused once m + 1 == M)
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        const double ar = c2r + dzr, ai = c2i + dzi;
        const double xr = ar * dzr, yr = ai * dzi;
        const double xi = ar * dzi, yi = ai * dzr;
        dzr = (xr - yr) + dcr;
        dzi = (xi + yi) + dci;
        ++m;
        const double zr = nz.x + dzr, zi = nz.y + dzi;
        const double mg = zr * zr + zi * zi;
        if (mg >= 4.0) {
            count = i;
            mag = mg;
            break;
        }
        const double dm = dzr * dzr + dzi * dzi;
        if (mg < dm || m == M) {   // rebase: the pixel's own z becomes its offset from Z_0 = 0
            dzr = zr;
            dzi = zi;
            m = 0u;
            c2r = 0.0;
            c2i = 0.0;
            nz = p.z1;
        } else {
            c2r = nz.z;
            c2i = nz.w;
            nz = pre;
        }
        pre = p.orbit[m + 2u < M ? m + 2u : M];
    }
    const size_t o = (size_t)lr * p.ncols + lc;
    if (p.counts) p.counts[o] = count;
    if (p.bytes) p.bytes[o] = quantise(count, p.mrd, p.quant_wide, p.quant_rcp);
    if (p.smooth) p.smooth[o] = smooth_value(count, mag);
}

}  // namespace mbk
