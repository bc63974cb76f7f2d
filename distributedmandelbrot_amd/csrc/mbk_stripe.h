// mbk_stripe.h -- stripe-average colouring for plain views (include/mbk.h, "Stripe-average colouring"): a statistic taken
// along a pixel's own orbit, the mean of 1/2 + 1/2 sin(s arg z_k), interpolated across the escape bands so that the picture is
// continuous.  For an integer density s, sin(s arg z) is the imaginary part of (z / |z|)^s: one square root, two divisions and
// s - 1 complex products, every one correctly rounded and none from libm, so the accumulated state is the same on the device,
// on the host and in numpy on every bit.  Only the interpolation weight of the value takes logarithms.  The term
// (stripe_term), the value (stripe_value) and the shade of a sample (stripe_shade) are __host__ __device__ functions that the
// kernel and the host twins share.
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own):
//   r = fl(sqrt(mag)), u = (fl(zr / r), fl(zi / r)), p = u, then s - 1 times p <- (fl(fl(p.r u.r) - fl(p.i u.i)),
//   fl(fl(p.r u.i) + fl(p.i u.r))); t = fl(0.5 + fl(0.5 p.i)); t = 0.5 unless 0 < mag < inf.
// Division and square root are the compiler's correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup around
// v_rcp_f64, v_rsq_f64 with its two refinement steps): no fast-math, no rcp shortcut.
//
// The kernel is the two-pass form of the distance kernel (mbk_distance.h): the counts come from the escape kernels, launched
// first and unchanged; a lane runs exactly its n steps with no bailout test -- the step counter is wave-uniform and a lane
// leaves by an integer compare against its own n -- and then the run-on to the large radius with its test.  mag_k comes from
// the squares the step forms anyway.  s and skip are launch-uniform, so the product loop's trip count and the test of the
// leading points left out are scalar.  One accumulator: the mean without the last term is formed from S - t_last.
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_distance.h"

namespace mbk {

constexpr uint32_t kStripeDensityMax = 16u;
constexpr double kStripeLB = 32.0 * 0x1.62e42fefa39efp-1;   // the binary64 nearest 32 ln 2 (a power of two times the nearest of ln 2)

// The term of one orbit point from z and mag = fl(fl(zr^2) + fl(zi^2)); 1 <= s <= 16.
__host__ __device__ inline double stripe_term(double zr, double zi, double mag, uint32_t s)
{
    const bool flat = !(mag > 0.0) || mag == INFINITY;   // NaN, 0, overflow
    const double r = sqrt(mag);
    const double ur = zr / r, ui = zi / r;
    double pr = ur, pi = ui;
    for (uint32_t j = 1u; j < s; ++j) {
        const double m0 = pr * ur, m1 = pi * ui, m2 = pr * ui, m3 = pi * ur;
        pr = m0 - m1;
        pi = m2 + m3;
    }
    const double h = 0.5 * pi;
    const double t = 0.5 + h;
    return flat ? 0.5 : t;
}

// The value of a pixel from its exact state: 0 for a pixel that never escaped, 0.5 with no term, S with one; otherwise
// a0 + (a1 - a0) d between the mean without the last term and the mean with it, d = 1 - log2(ln mag / (32 ln 2)) clamped to
// [0, 1] (0 for a NaN: mag = inf).  Never a NaN.
__host__ __device__ inline double stripe_value(double S, double t_last, int32_t cnt, double mag, int32_t count)
{
    if (count <= 0) return 0.0;
    if (cnt <= 0) return 0.5;
    if (cnt == 1) return S;
    const double a1 = S / (double)cnt;
    const double rest = S - t_last;
    const double a0 = rest / (double)(cnt - 1);
    const double l = log(mag);
    const double q = l / kStripeLB;
    const double g = log2(q);
    double d = 1.0 - g;
    if (!(d >= 0.0)) d = 0.0;
    if (d > 1.0) d = 1.0;
    const double diff = a1 - a0;
    const double w = diff * d;
    return a0 + w;
}

// The brightness q in [0, 256] of a sample with value v: w = fl(0.5 + fl(gain fl(v - 0.5))) clamped to [0, 1],
// t = fl(lo + fl(fl(1 - lo) w)); 256 from t >= 1 up, floor(256 t) below (exact).  lo in [0, 1], gain in [0, 2^10], v never NaN.
__host__ __device__ inline uint32_t stripe_shade(double v, double lo, double gain)
{
    const double c = v - 0.5;
    const double g = gain * c;
    double w = 0.5 + g;
    if (!(w >= 0.0)) w = 0.0;
    if (w > 1.0) w = 1.0;
    const double span = 1.0 - lo;
    const double m = span * w;
    const double t = lo + m;
    if (!(t > 0.0)) return 0u;
    if (t >= 1.0) return 256u;
    return (uint32_t)(t * 256.0);
}

// One step of z.  (a, b) = (zr^2, zi^2) come in from the previous step and go out for the next one and for mag.
template <bool kFmaDouble>
__host__ __device__ __forceinline__ void stripe_step(double &zr, double &zi, double &a, double &b, double cr, double ci)
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

// The exact state of a pixel beside its count n: all zero where n = 0.
struct StripeState {
    double S, t_last, mag;
    int32_t N, cnt;
};

// The replay of one pixel whose count is n > 0: n steps, then the run-on.  The sum takes the points skip + 1 .. N.
template <bool kFmaDouble>
__host__ __device__ inline StripeState stripe_replay(double cr, double ci, int32_t n, uint32_t s, uint32_t skip)
{
    double zr = cr, zi = ci, a = zr * zr, b = zi * zi;
    double S = 0.0, t = 0.0, mag = a + b;
    uint32_t k = 0u;
    while (k < (uint32_t)n) {
        stripe_step<kFmaDouble>(zr, zi, a, b, cr, ci);
        mag = a + b;
        if (++k > skip) {
            t = stripe_term(zr, zi, mag, s);
            S += t;
        }
    }
    for (int extra = 0; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
        stripe_step<kFmaDouble>(zr, zi, a, b, cr, ci);
        mag = a + b;
        if (++k > skip) {
            t = stripe_term(zr, zi, mag, s);
            S += t;
        }
    }
    StripeState st;
    st.S = S;
    st.t_last = t;
    st.mag = mag;
    st.N = (int32_t)k;
    st.cnt = k > skip ? (int32_t)(k - skip) : 0;
    return st;
}

struct StripeArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;          // 8x8 blocks per block row (1-D grid, row-major)
    uint32_t density, skip;
    const int32_t *counts_in;   // the escape kernels' counts (window layout)
    double *value;
    double *state;              // may be null; px x (S, t_last, mag), then px x N and px x cnt as int32: 32 bytes per pixel
    uint64_t px;
};

template <bool kFmaDouble>
__global__ __launch_bounds__(64) void stripe_kernel(const StripeArgs p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    const bool live = lc < p.ncols && lr < p.nrows;
    const size_t o = live ? (size_t)lr * p.ncols + lc : 0u;
    int32_t *const st_n = p.state ? reinterpret_cast<int32_t *>(p.state + 3u * p.px) : nullptr;
    int32_t n = 0;
    if (live) n = p.counts_in[o];
    if (__ballot(n > 0) == 0ull) {   // nothing escaped here: the interior, and the blocks outside the window
        if (live) {
            p.value[o] = 0.0;
            if (p.state) {
                p.state[o] = 0.0;
                p.state[p.px + o] = 0.0;
                p.state[2u * p.px + o] = 0.0;
                st_n[o] = 0;
                st_n[p.px + o] = 0;
            }
        }
        return;
    }
    const double cr = axis_value(p.re, p.col0 + (live ? lc : 0u));
    const double ci = axis_value(p.im, p.row0 + (live ? lr : 0u));
    const uint32_t s = p.density, skip = p.skip;
    double zr = cr, zi = ci;
    double a = zr * zr, b = zi * zi;
    double S = 0.0, t = 0.0;
    int32_t nmax = n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t other = __shfl_xor(nmax, off);
        nmax = other > nmax ? other : nmax;
    }
    nmax = __builtin_amdgcn_readfirstlane(nmax);
    for (int32_t k = 0; k < nmax; ++k) {
        if (k < n) {
            stripe_step<kFmaDouble>(zr, zi, a, b, cr, ci);
            if ((uint32_t)k >= skip) {   // (scalar: the point's index k + 1 lies past the leading ones left out)
                t = stripe_term(zr, zi, a + b, s);
                S += t;
            }
        }
    }
    double mag = a + b;
    uint32_t N = (uint32_t)n;
    if (n > 0) {
        for (int extra = 0; extra < kDistanceRunOn && !(mag >= kDistanceRadius2); ++extra) {
            stripe_step<kFmaDouble>(zr, zi, a, b, cr, ci);
            mag = a + b;
            if (++N > skip) {
                t = stripe_term(zr, zi, mag, s);
                S += t;
            }
        }
    }
    if (!live) return;
    if (n <= 0) mag = 0.0;   // (a pixel of the set in a block that is not: the all-zero state)
    const int32_t cnt = N > skip ? (int32_t)(N - skip) : 0;
    p.value[o] = stripe_value(S, t, cnt, mag, n);
    if (p.state) {
        p.state[o] = S;
        p.state[p.px + o] = t;
        p.state[2u * p.px + o] = mag;
        st_n[o] = (int32_t)N;
        st_n[p.px + o] = cnt;
    }
}

}   // namespace mbk
