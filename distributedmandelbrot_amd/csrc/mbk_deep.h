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
// rebase) comes with the arguments.  The pixel set-up and the cursor that holds m and the entries are mbk_deep_cursor.h's, which
// the deep kernels use; the start state, the plain step and the rebase test below are shared with the other binary64 kernels
// and their host twins.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbk_deep_cursor.h"

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

// the plain step with c2 = 2 Z_m
__host__ __device__ __forceinline__ void deep_plain_step(double c2r, double c2i, double dcr, double dci, double &dzr, double &dzi)
{
    const double ar = c2r + dzr, ai = c2i + dzi;
    const double xr = ar * dzr, yr = ai * dzi;
    const double xi = ar * dzi, yi = ai * dzr;
    dzr = (xr - yr) + dcr;
    dzi = (xi + yi) + dci;
}

// The start state, shared by the kernels and the host twins: z_0 = c = fl(Z_1 + dc) and dz = dc at m = 1 -- or, for an orbit of
// length 1 (no Z_2), rebased at once: dz = z_0 at m = 0.  Returns m.
__host__ __device__ __forceinline__ uint32_t deep_start(double z1r, double z1i, uint32_t M, double dcr, double dci, double &dzr, double &dzi,
                                                        double &zr, double &zi)
{
    zr = z1r + dcr;
    zi = z1i + dci;
    if (M == 1u) {
        dzr = zr;
        dzi = zi;
        return 0u;
    }
    dzr = dcr;
    dzi = dci;
    return 1u;
}

// The rebase comparison, |z|^2 < |dz|^2 with mg = |z|^2 (wide_rebase of mbk_deep_wide.h is its wide form).  A pixel also rebases
// where the table ends: m == M, the cursor's last().
__host__ __device__ __forceinline__ bool deep_rebase(double mg, double dzr, double dzi)
{
    const double dm = dzr * dzr + dzi * dzi;
    return mg < dm;
}

// The escape loop of the sample at offset dc: its count and |z|^2 at the escaping step (0, 0 for a sample that stays).  Written
// once for deep_view_kernel and the refine kernel of an adaptive render (mbk_deep_adaptive.h), whose samples must be the bits
// this launch stores.  The four escape functions return by value on purpose: with count and mag as reference out-parameters the
// stores through them sit in the loop while the function is optimised on its own, before it is inlined, and deep_view_kernel's
// loop comes out restructured (profiles/refine_walk/README.md).
__device__ __forceinline__ EscapeSample deep_escape(const DeepArgs &p, double dcr, double dci)
{
    double dzr, dzi, zr, zi;
    OrbitCursor<double4> c(p.orbit, p.z1, p.M, deep_start(p.z1.x, p.z1.y, p.M, dcr, dci, dzr, dzi, zr, zi));
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        deep_plain_step(c.cur.z, c.cur.w, dcr, dci, dzr, dzi);
        c.step();
        zr = c.nz.x + dzr;
        zi = c.nz.y + dzi;
        const double mg = zr * zr + zi * zi;
        if (mg >= 4.0) {
            count = i;
            mag = mg;
            break;
        }
        if (deep_rebase(mg, dzr, dzi) || c.last()) {
            dzr = zr;
            dzi = zi;
            c.rebased();
        } else {
            c.advanced();
        }
        c.prefetch();
    }
    return EscapeSample{count, mag};
}

__global__ __launch_bounds__(64) void deep_view_kernel(DeepArgs p)
{
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const EscapeSample e = deep_escape(p, px.dcr, px.dci);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = e.count;
    if (p.bytes) p.bytes[o] = quantise(e.count, p.mrd, p.quant_wide, p.quant_rcp);
    if (p.smooth) p.smooth[o] = smooth_value(e.count, e.mag);
}

}  // namespace mbk
