// mbk_render.h -- views to RGBA8 images (include/mbk.h, "Rendering"): the colour of one sample and the resolve of a pixel's
// s x s samples, written once as __host__ __device__ functions that the resolve kernel and mbk_render_resolve_host share, and
// the kernel itself (six rules for the binary64 samples: smooth, distance, equalised, interior, relief, stripe).  The samples come from the existing escape kernels, launched on a band's window; nothing here iterates.
//
// Everything after the samples is integer arithmetic or exact binary64: t = fl(fl(nu * scale) + offset) are two rounded
// operations (the translation unit is compiled with -ffp-contract=off), floor(t) and (t - floor(t)) * 256 are exact for
// 0 <= t < 2^52, and k mod n is computed through a binary64 quotient estimate that is corrected to the exact remainder.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <hip/hip_runtime.h>

#include "mbk_histogram.h"
#include "mbk_relief.h"
#include "mbk_stripe.h"

namespace mbk {

// A palette as the kernel sees it: n RGBA8 entries packed into little-endian words (R in bits 0..7, A in 24..31).
struct RenderPalette {
    const uint32_t *entries;
    uint32_t n;
    double n_rcp;      // fl(1 / n): the quotient estimate of index_mod
    uint32_t inside;   // MBK_RENDER_SMOOTH: the colour of a sample whose count is 0
    double scale, offset;
    const double *lut;   // MBK_RENDER_EQUALIZED: the equalisation table, lut_mrd + 2 entries
    uint32_t lut_mrd;
    uint32_t unknown, outside;   // interior renders: the colours of a sample with no period and of one that escapes
    double light_x, light_y, height;   // relief renders (mbk.h "Relief shading")
    double stripe_lo, stripe_gain;     // stripe renders (mbk.h "Stripe-average colouring")
};

// How a binary64 sample becomes a colour: the three rules of the sources that share the (count, value) sample layout.
// kRuleInterior (mbk.h "Interior views") reads a third array, the periods, beside the same two; kRuleRelief (mbk.h "Relief
// shading") the normals, two binary64 per sample; kRuleStripe (mbk.h "Stripe-average colouring") the stripe values, one.
enum RenderRule { kRuleSmooth = 0, kRuleDistance = 1, kRuleEqualized = 2, kRuleInterior = 3, kRuleRelief = 4, kRuleStripe = 5 };

// Two colour channels at a time: a word holds channels 0 and 2 (or 1 and 3) in its 16-bit halves.
__host__ __device__ inline uint32_t render_even(uint32_t c) { return c & 0x00ff00ffu; }
__host__ __device__ inline uint32_t render_odd(uint32_t c) { return (c >> 8) & 0x00ff00ffu; }

// (p0 (256 - f) + p1 f + 128) >> 8 per channel, 0 <= f <= 255.  A half holds at most 255 * 256 + 128 < 2^16: no carry
// crosses into the other channel.
__host__ __device__ inline uint32_t render_blend(uint32_t p0, uint32_t p1, uint32_t f)
{
    const uint32_t g = 256u - f;
    const uint32_t even = ((render_even(p0) * g + render_even(p1) * f + 0x00800080u) >> 8) & 0x00ff00ffu;
    const uint32_t odd = ((render_odd(p0) * g + render_odd(p1) * f + 0x00800080u) >> 8) & 0x00ff00ffu;
    return even | (odd << 8);
}

// k mod n for an integer-valued 0 <= k < 2^52 and 2 <= n <= 65536.  q = floor(fl(k * fl(1/n))) is within 1 of the true
// quotient (relative error < 2^-51, k / n < 2^51), r = k - q n is exact in binary64 (|r| < 2 n, one fma), and one
// correction either way lands in [0, n).
__host__ __device__ inline uint32_t render_index_mod(double k, uint32_t n, double n_rcp)
{
    const double q = floor(k * n_rcp);
    double r = fma(-q, (double)n, k);
    if (r < 0.0) r += (double)n;
    if (r >= (double)n) r -= (double)n;
    return (uint32_t)r;
}

// The colour of one MBK_RENDER_SMOOTH sample (mbk.h: decided on the count, not on nu).
__host__ __device__ inline uint32_t render_colour_smooth(const RenderPalette &p, const uint32_t *entries, int32_t count, double nu)
{
    if (count == 0) return p.inside;
    double t = nu * p.scale;
    t = t + p.offset;
    if (!(t >= 0.0 && t < 0x1p52)) t = 0.0;   // negative, -inf, NaN; and t >= 2^52, which no launch's nu can reach
    const double k = floor(t);
    const uint32_t f = (uint32_t)((t - k) * 256.0);
    const uint32_t i0 = render_index_mod(k, p.n, p.n_rcp);
    const uint32_t i1 = i0 + 1u == p.n ? 0u : i0 + 1u;
    return render_blend(entries[i0], entries[i1], f);
}

// The colour of one MBK_RENDER_DISTANCE sample: the smooth rule with the distance estimate in place of nu, except that the
// palette does not wrap: t >= n - 1 (+inf included) is the last entry.  t < n - 1 <= 65535 below: floor and f are exact.
__host__ __device__ inline uint32_t render_colour_distance(const RenderPalette &p, const uint32_t *entries, int32_t count, double de)
{
    if (count == 0) return p.inside;
    double t = de * p.scale;
    t = t + p.offset;
    if (!(t >= 0.0)) t = 0.0;   // negative, NaN
    if (t >= (double)(p.n - 1u)) return entries[p.n - 1u];
    const double k = floor(t);
    const uint32_t f = (uint32_t)((t - k) * 256.0);
    const uint32_t i0 = (uint32_t)k;
    return render_blend(entries[i0], entries[i0 + 1u], f);
}

// The colour of one MBK_RENDER_EQUALIZED sample: nu through the equalisation table (mbk_histogram.h), then the distance rule
// with that value in place of de.  The table is read from global memory: up to 8 MiB does not fit LDS, and its accesses are
// as coherent as the image.
__host__ __device__ inline uint32_t render_colour_equalized(const RenderPalette &p, const uint32_t *entries, int32_t count, double nu)
{
    if (count == 0) return p.inside;
    return render_colour_distance(p, entries, count, equalize_value(p.lut, p.lut_mrd, nu));
}

// R, G and B of `base` scaled by f / 256, 0 <= f <= 256: (channel f + 128) >> 8.  Alpha is the base's.
__host__ __device__ inline uint32_t render_dim(uint32_t base, uint32_t f)
{
    const uint32_t even = ((render_even(base) * f + 0x00800080u) >> 8) & 0x00ff00ffu;   // R, B
    const uint32_t green = ((((base >> 8) & 0xffu) * f + 128u) >> 8) & 0xffu;
    return even | (green << 8) | (base & 0xff000000u);
}

// The colour of one interior sample: `outside` if it escapes, `unknown` without a period; otherwise the palette entry of the
// period (cyclic, 1 <= n <= 65536) with R, G, B scaled by f / 256, f = 256 from t = fl(de scale) >= 1 up (+inf included),
// floor(256 t) below (exact: t < 1).  de is never NaN or negative.  Alpha is the entry's.
__host__ __device__ inline uint32_t render_colour_interior(const RenderPalette &p, const uint32_t *entries, int32_t count, int32_t period,
                                                           double de)
{
    if (count > 0) return p.outside;
    if (period <= 0) return p.unknown;
    const uint32_t base = entries[(uint32_t)(period - 1) % p.n];
    const double t = de * p.scale;
    const uint32_t f = t >= 1.0 ? 256u : (uint32_t)(t * 256.0);
    return render_dim(base, f);
}

// The colour of one relief sample: `inside`, unshaded, if the count is 0; otherwise the MBK_RENDER_SMOOTH colour with R, G, B
// scaled by q / 256, q the shade of the sample's normal (relief_shade).
__host__ __device__ inline uint32_t render_colour_relief(const RenderPalette &p, const uint32_t *entries, int32_t count, double nu, double nx,
                                                         double ny)
{
    if (count == 0) return p.inside;
    return render_dim(render_colour_smooth(p, entries, count, nu), relief_shade(nx, ny, p.light_x, p.light_y, p.height));
}

// The colour of one stripe sample: `inside`, unshaded, if the count is 0; otherwise the MBK_RENDER_SMOOTH colour with R, G, B
// scaled by q / 256, q the shade of the sample's stripe average (stripe_shade).
__host__ __device__ inline uint32_t render_colour_stripe(const RenderPalette &p, const uint32_t *entries, int32_t count, double nu, double v)
{
    if (count == 0) return p.inside;
    return render_dim(render_colour_smooth(p, entries, count, nu), stripe_shade(v, p.stripe_lo, p.stripe_gain));
}

template <int RULE>
__host__ __device__ inline uint32_t render_colour(const RenderPalette &p, const uint32_t *entries, int32_t count, double value)
{
    if constexpr (RULE == kRuleDistance)
        return render_colour_distance(p, entries, count, value);
    else if constexpr (RULE == kRuleEqualized)
        return render_colour_equalized(p, entries, count, value);
    else
        return render_colour_smooth(p, entries, count, value);
}

// The sum of a pixel's sample colours, two channels to a word (8 x 8 x 255 < 2^16), and its rounded mean
// (2 sum + s^2) / (2 s^2), rounded down: round half up, the identity for s = 1.
struct RenderSum {
    uint32_t even = 0u, odd = 0u;
    __host__ __device__ inline void add(uint32_t c)
    {
        even += render_even(c);
        odd += render_odd(c);
    }
    __host__ __device__ inline uint32_t mean(uint32_t s2) const
    {
        const uint32_t d = 2u * s2;
        const uint32_t c0 = (2u * (even & 0xffffu) + s2) / d, c2 = (2u * (even >> 16) + s2) / d;
        const uint32_t c1 = (2u * (odd & 0xffffu) + s2) / d, c3 = (2u * (odd >> 16) + s2) / d;
        return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
    }
};

// One band of a render: the samples of `ncols x nrows` output pixels, row pitch `pitch` samples (>= ncols * S), and where the
// pixels go: out + (row * out_pitch + col) words.
struct RenderArgs {
    const int32_t *counts;   // MBK_RENDER_SMOOTH
    const double *smooth;
    const int32_t *period;   // kRuleInterior
    const double *normal;    // kRuleRelief: [sample][2]
    const double *stripe;    // kRuleStripe: [sample]
    const uint8_t *bytes;    // MBK_RENDER_BYTES
    uint32_t *out;
    uint64_t pitch, out_pitch;
    uint32_t ncols, nrows;
    uint32_t chunks_x;       // pieces of 256 lanes' output pixels per row
    uint32_t lds_palette;    // the palette is staged in (dynamic) LDS
    RenderPalette pal;
};

constexpr uint32_t kRenderThreads = 256;
constexpr uint32_t kRenderBytesPx = 4;   // MBK_RENDER_BYTES: adjacent output pixels per lane (S * 4 sample bytes per load)
constexpr uint32_t kRenderLdsEntries = 16384;   // palettes up to 64 KiB of the CU's 160 KiB sit in LDS

// S samples of one sample row, starting at a multiple of S in a row whose pitch is a multiple of S: for even S the pairs are
// 16-byte (nu) / 8-byte (count) aligned whenever the band's base is, which hipMalloc guarantees.
template <int S>
__device__ inline void render_load_smooth(const RenderArgs &a, uint64_t at, double (&nu)[S], int32_t (&cnt)[S])
{
    if constexpr (S % 2 == 0) {
        const double2 *pn = reinterpret_cast<const double2 *>(a.smooth + at);
        const int2 *pc = reinterpret_cast<const int2 *>(a.counts + at);
#pragma unroll
        for (int k = 0; k < S / 2; ++k) {
            const double2 v = pn[k];
            const int2 c = pc[k];
            nu[2 * k] = v.x;
            nu[2 * k + 1] = v.y;
            cnt[2 * k] = c.x;
            cnt[2 * k + 1] = c.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            nu[k] = a.smooth[at + k];
            cnt[k] = a.counts[at + k];
        }
    }
}

// The resolve kernel.  A workgroup walks pieces of a row of the band: 256 lanes on 256 (SMOOTH) or 1024 (BYTES, four to a
// lane) adjacent output pixels, so that a wave's loads cover one contiguous stretch of each sample row and its stores one
// contiguous stretch of the image.  The grid is sized to the chip and every workgroup takes pieces in turn, which is what
// makes staging the palette in LDS worth its loads.  Pure streaming: s^2 x (12 | 1) bytes in, 4 bytes out per pixel.
// RULE (with SMOOTH): what the binary64 samples are -- nu, distance estimates (render_colour_distance) or nu for the
// equalisation table (render_colour_equalized); same loads, same layout.  kRuleInterior, kRuleRelief and kRuleStripe read one
// more array per sample (the periods; the normals, 16 bytes; the stripe values, 8) straight from global memory.
template <bool SMOOTH, int S, int RULE = kRuleSmooth>
__global__ __launch_bounds__(kRenderThreads) void render_resolve_kernel(const RenderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_palette[];
    const uint32_t *entries = a.pal.entries;
    if (a.lds_palette) {
        for (uint32_t k = threadIdx.x; k < a.pal.n; k += kRenderThreads) s_palette[k] = a.pal.entries[k];
        __syncthreads();
        entries = s_palette;
    }
    const uint64_t pieces = (uint64_t)a.chunks_x * a.nrows;
    for (uint64_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
        const uint32_t row = (uint32_t)(piece / a.chunks_x), cx = (uint32_t)(piece % a.chunks_x);
        uint32_t *out_row = a.out + (uint64_t)row * a.out_pitch;
        if constexpr (SMOOTH) {
            const uint32_t col = cx * kRenderThreads + threadIdx.x;
            if (col >= a.ncols) continue;
            RenderSum sum;
#pragma unroll
            for (int sy = 0; sy < S; ++sy) {
                double nu[S];
                int32_t cnt[S];
                const uint64_t at = ((uint64_t)row * S + sy) * a.pitch + (uint64_t)col * S;
                render_load_smooth<S>(a, at, nu, cnt);
#pragma unroll
                for (int sx = 0; sx < S; ++sx) {
                    if constexpr (RULE == kRuleInterior)
                        sum.add(render_colour_interior(a.pal, entries, cnt[sx], a.period[at + sx], nu[sx]));
                    else if constexpr (RULE == kRuleRelief) {   // (16-byte aligned: the band's base is, and a sample is 16 bytes)
                        const double2 nv = reinterpret_cast<const double2 *>(a.normal)[at + sx];
                        sum.add(render_colour_relief(a.pal, entries, cnt[sx], nu[sx], nv.x, nv.y));
                    } else if constexpr (RULE == kRuleStripe)
                        sum.add(render_colour_stripe(a.pal, entries, cnt[sx], nu[sx], a.stripe[at + sx]));
                    else
                        sum.add(render_colour<RULE>(a.pal, entries, cnt[sx], nu[sx]));
                }
            }
            out_row[col] = sum.mean(S * S);
        } else {
            const uint32_t col = (cx * kRenderThreads + threadIdx.x) * kRenderBytesPx;
            if (col >= a.ncols) continue;
            const uint32_t npx = a.ncols - col < kRenderBytesPx ? a.ncols - col : kRenderBytesPx;
            RenderSum sum[kRenderBytesPx];
            if (npx == kRenderBytesPx) {
#pragma unroll
                for (int sy = 0; sy < S; ++sy) {
                    uint8_t b[kRenderBytesPx * S];   // an unaligned load of 4 S bytes (a sample row's pitch may be odd)
                    __builtin_memcpy(b, a.bytes + ((uint64_t)row * S + sy) * a.pitch + (uint64_t)col * S, sizeof(b));
#pragma unroll
                    for (int k = 0; k < (int)kRenderBytesPx * S; ++k) sum[k / S].add(entries[b[k]]);
                }
                uint32_t px[kRenderBytesPx];
#pragma unroll
                for (int k = 0; k < (int)kRenderBytesPx; ++k) px[k] = sum[k].mean(S * S);
                uint32_t *dst = out_row + col;
                if (((uintptr_t)dst & 15u) == 0u) {
                    *reinterpret_cast<uint4 *>(dst) = make_uint4(px[0], px[1], px[2], px[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < (int)kRenderBytesPx; ++k) dst[k] = px[k];
                }
            } else {   // the last one to three pixels of a row
                for (uint32_t k = 0; k < npx; ++k) {
                    RenderSum one;
                    for (int sy = 0; sy < S; ++sy)
                        for (int sx = 0; sx < S; ++sx)
                            one.add(entries[a.bytes[((uint64_t)row * S + sy) * a.pitch + (uint64_t)(col + k) * S + sx]]);
                    out_row[col + k] = one.mean(S * S);
                }
            }
        }
    }
}

template <bool SMOOTH, int RULE = kRuleSmooth>
inline void launch_resolve(uint32_t s, dim3 grid, size_t lds, hipStream_t stream, const RenderArgs &a)
{
    const dim3 block(kRenderThreads);
    switch (s) {
        case 1: hipLaunchKernelGGL((render_resolve_kernel<SMOOTH, 1, RULE>), grid, block, lds, stream, a); break;
        case 2: hipLaunchKernelGGL((render_resolve_kernel<SMOOTH, 2, RULE>), grid, block, lds, stream, a); break;
        case 3: hipLaunchKernelGGL((render_resolve_kernel<SMOOTH, 3, RULE>), grid, block, lds, stream, a); break;
        case 4: hipLaunchKernelGGL((render_resolve_kernel<SMOOTH, 4, RULE>), grid, block, lds, stream, a); break;
        default: hipLaunchKernelGGL((render_resolve_kernel<SMOOTH, 8, RULE>), grid, block, lds, stream, a); break;
    }
}

// The same rule on the host, for caller-supplied samples of (width * s) x (height * s): mbk_render_resolve_host.
inline void render_resolve_host(const RenderPalette &pal, bool smooth_source, uint32_t s, uint32_t width, uint32_t height,
                                const int32_t *counts, const uint8_t *bytes, const double *smooth, uint8_t *rgba,
                                int rule = kRuleSmooth, const int32_t *period = nullptr, const double *normal = nullptr,
                                const double *stripe = nullptr)
{
    const uint64_t pitch = (uint64_t)width * s;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            RenderSum sum;
            for (uint32_t sy = 0; sy < s; ++sy)
                for (uint32_t sx = 0; sx < s; ++sx) {
                    const uint64_t at = ((uint64_t)y * s + sy) * pitch + (uint64_t)x * s + sx;
                    sum.add(!smooth_source            ? pal.entries[bytes[at]]
                            : rule == kRuleInterior  ? render_colour_interior(pal, pal.entries, counts[at], period[at], smooth[at])
                            : rule == kRuleRelief    ? render_colour_relief(pal, pal.entries, counts[at], smooth[at], normal[2u * at], normal[2u * at + 1u])
                            : rule == kRuleStripe    ? render_colour_stripe(pal, pal.entries, counts[at], smooth[at], stripe[at])
                            : rule == kRuleDistance  ? render_colour_distance(pal, pal.entries, counts[at], smooth[at])
                            : rule == kRuleEqualized ? render_colour_equalized(pal, pal.entries, counts[at], smooth[at])
                                                     : render_colour_smooth(pal, pal.entries, counts[at], smooth[at]));
                }
            const uint32_t c = sum.mean(s * s);
            uint8_t *o = rgba + ((uint64_t)y * width + x) * 4u;
            o[0] = (uint8_t)c;
            o[1] = (uint8_t)(c >> 8);
            o[2] = (uint8_t)(c >> 16);
            o[3] = (uint8_t)(c >> 24);
        }
}

}   // namespace mbk
