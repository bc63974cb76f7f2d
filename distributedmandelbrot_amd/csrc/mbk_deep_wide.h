// mbk_deep_wide.h -- extended-range deep views (include/mbk.h, "Extended-range deep views"): the perturbation step of
// mbk_deep.h with every number carried as a binary64 mantissa pair and one int32 exponent, so that neither the offsets nor
// the reference orbit are bound to binary64's exponent range.  dz = (wr, wi) 2^q with max(|wr|, |wi|) in [0.5, 1) (or
// (0, 0, kWideZeroExp)); Z_m = (xr, xi) 2^xe from the wide table (mbk_deep_orbit.h); dc = (dcr, dci) 2^exp2.
//
// A step aligns the two terms of each sum to the larger exponent with ldexp (exact unless the result is subnormal), adds and
// multiplies the mantissas in strict binary64 -- the translation unit is compiled -ffp-contract=off -- and renormalises with
// frexp's exponent.  Scaling by a power of two is exact, so wherever the plain step meets no subnormal the two store the
// same bits.  ldexp and frexp go through the builtins that become v_ldexp_f64 / v_frexp_exp_i32_f64; fp64 denormals are
// honoured on the device (the default), and the contract's one-rounding rule for subnormal results relies on that.
//
// The kernel has the shape of deep_view_kernel: one lane per pixel, one 8x8 block per single-wave workgroup in image order,
// an ordinary divergent loop bounded by mrd (a lane that escapes leaves EXEC), no wave-uniform value taken from a lane, the
// entry the next step needs loaded one step ahead -- the pixel and the cursor of mbk_deep_cursor.h.  wide_count_host runs the
// same start and step functions on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "mbk_deep_cursor.h"
#include "mbk_deep_orbit.h"

namespace mbk {

// sh(x, k) = ldexp(x, max(k, -1200))
__host__ __device__ inline double wide_sh(double x, int32_t k) { return __builtin_ldexp(x, k < -1200 ? -1200 : k); }

// frexp's exponent of a finite a > 0 (subnormals included)
__host__ __device__ inline int32_t wide_exp(double a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_frexp_exp(a);
#else
    int e;
    (void)std::frexp(a, &e);
    return e;
#endif
}

__host__ __device__ inline int32_t wide_max(int32_t a, int32_t b) { return a > b ? a : b; }

// norm(v, e): the larger |component| into [0.5, 1)
__host__ __device__ inline void wide_norm(double vr, double vi, int32_t e, double &wr, double &wi, int32_t &q)
{
    const double ar = __builtin_fabs(vr), ai = __builtin_fabs(vi);
    const double mx = ar > ai ? ar : ai;
    if (mx == 0.0) {
        wr = 0.0;
        wi = 0.0;
        q = kWideZeroExp;
        return;
    }
    const int32_t s = wide_exp(mx);
    wr = __builtin_ldexp(vr, -s);
    wi = __builtin_ldexp(vi, -s);
    q = e + s;
}

// steps (a) .. (d): dz = (2 Z_m + dz) dz + dc with (xr, xi, xe) the entry m
__host__ __device__ inline void wide_step(double xr, double xi, int32_t xe, double dcr, double dci, int32_t exp2, double &wr,
                                          double &wi, int32_t &q)
{
    const int32_t x1 = xe + 1, g = wide_max(x1, q);
    const double Ar = wide_sh(xr, x1 - g) + wide_sh(wr, q - g);
    const double Ai = wide_sh(xi, x1 - g) + wide_sh(wi, q - g);
    const double ur = Ar * wr, vr = Ai * wi;
    const double ui = Ar * wi, vi = Ai * wr;
    const double pr = ur - vr, pi = ui + vi;
    const int32_t pe = g + q, h = wide_max(pe, exp2);
    const double Nr = wide_sh(pr, pe - h) + wide_sh(dcr, exp2 - h);
    const double Ni = wide_sh(pi, pe - h) + wide_sh(dci, exp2 - h);
    wide_norm(Nr, Ni, h, wr, wi, q);
}

// step (e): z = Z_m + dz as (zr, zi) 2^t with (xr, xi, xe) the entry m, and mg = |(zr, zi)|^2
__host__ __device__ inline void wide_z(double xr, double xi, int32_t xe, double wr, double wi, int32_t q, double &zr,
                                       double &zi, int32_t &t, double &mg)
{
    t = wide_max(xe, q);
    zr = wide_sh(xr, xe - t) + wide_sh(wr, q - t);
    zi = wide_sh(xi, xe - t) + wide_sh(wi, q - t);
    const double a = zr * zr, b = zi * zi;
    mg = a + b;
}

// |z|^2 as a plain binary64 (step (e)'s mag)
__host__ __device__ inline double wide_mag(double mg, int32_t t) { return __builtin_ldexp(mg, 2 * wide_max(t, -600)); }

// step (g)'s comparison: |z|^2 < |dz|^2, both on z's exponent
__host__ __device__ inline bool wide_rebase(double mg, double wr, double wi, int32_t q, int32_t t)
{
    const double a = wr * wr, b = wi * wi;
    const double dm = a + b;
    return mg < __builtin_ldexp(dm, 2 * wide_max(q - t, -600));
}

struct DeepWideArgs {
    const WideEntry *orbit;   // entries 0 .. M
    WideEntry z1;             // entry 1
    uint32_t M;               // the orbit's length (>= 1)
    int32_t exp2;
    double half_r, half_i;    // (W - 1) / 2, (H - 1) / 2: exact
    double step_r, step_i;    // fl(range_r / (W - 1)), fl(range_i / (H - 1)); 0 for a single column / row
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;        // 8x8 blocks per row of blocks
    int32_t mrd;
    uint32_t quant_wide;      // the quantiser of mbk_kernels.h (quantise)
    double quant_rcp;
    int32_t *counts;          // may be null
    uint8_t *bytes;           // may be null
    double *smooth;           // may be null
};

// The start state, shared by the kernels and the host twins: dz = norm(dc) and z_0 = c = Z_1 + dc (with its mg) at m = 1 -- or,
// for an orbit of length 1 (no Z_2), rebased at once: dz = norm(z_0) at m = 0.  Returns m.
__host__ __device__ __forceinline__ uint32_t wide_start(const WideEntry &z1, uint32_t M, double dcr, double dci, int32_t exp2, double &wr,
                                                        double &wi, int32_t &q, double &zr, double &zi, int32_t &t, double &mg)
{
    wide_norm(dcr, dci, exp2, wr, wi, q);
    wide_z(z1.xr, z1.xi, z1.xe, wr, wi, q, zr, zi, t, mg);
    if (M != 1u) return 1u;
    wide_norm(zr, zi, t, wr, wi, q);
    return 0u;
}

// The escape loop of the sample at offset dc 2^exp2: its count and |z|^2 at the escaping step as a plain binary64 (0, 0 for a
// sample that stays), by value as deep_escape (mbk_deep.h).  Written once for deep_wide_kernel and the refine kernel of an
// adaptive render (mbk_deep_wide_adaptive.h), whose samples must be the bits this launch stores.
__device__ __forceinline__ EscapeSample deep_wide_escape(const DeepWideArgs &p, double dcr, double dci)
{
    const int32_t exp2 = p.exp2;
    double wr, wi, zr, zi, mg;
    int32_t q, t;
    OrbitCursor<WideEntry> c(p.orbit, p.z1, p.M, wide_start(p.z1, p.M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg));
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        wide_step(c.cur.xr, c.cur.xi, c.cur.xe, dcr, dci, exp2, wr, wi, q);
        c.step();
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
    return EscapeSample{count, mag};
}

__global__ __launch_bounds__(64) void deep_wide_kernel(DeepWideArgs p)
{
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const EscapeSample e = deep_wide_escape(p, px.dcr, px.dci);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = e.count;
    if (p.bytes) p.bytes[o] = quantise(e.count, p.mrd, p.quant_wide, p.quant_rcp);
    if (p.smooth) p.smooth[o] = smooth_value(e.count, e.mag);
}

// One pixel on the host, from the functions the kernel uses: the count and |z|^2 at the escaping step (0 for count 0).
inline void wide_count_host(const std::vector<WideEntry> &orbit, uint32_t M, double dcr, double dci, int32_t exp2, int64_t mrd,
                            int32_t *count, double *mag)
{
    const WideEntry *Z = orbit.data();
    double wr, wi, zr, zi, mg;
    int32_t q, t;
    uint32_t m = wide_start(Z[1], M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg);
    *count = 0;
    *mag = 0.0;
    for (int64_t i = 1; i < mrd; ++i) {
        wide_step(Z[m].xr, Z[m].xi, Z[m].xe, dcr, dci, exp2, wr, wi, q);
        ++m;
        wide_z(Z[m].xr, Z[m].xi, Z[m].xe, wr, wi, q, zr, zi, t, mg);
        const double mgs = wide_mag(mg, t);
        if (mgs >= 4.0) {
            *count = (int32_t)i;
            *mag = mgs;
            return;
        }
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
        }
    }
}

}  // namespace mbk
