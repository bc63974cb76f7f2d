// mbk_deep_wide_adaptive.h -- adaptive supersampling of extended-range deep-view smooth renders (include/mbk.h, "Adaptive
// supersampling of extended-range deep views"): the refine kernel.  The base pass is the wide sample launch and the classify
// kernel is mbk_adaptive.h's, which works on samples and does not care what kind of view made them; what a wide view needs of
// its own is the kernel that computes the s x s fine samples of the listed pixels in the wide number system.
//
// The list is walked as deep_adaptive_refine_kernel walks it (a grid sized to the chip, chunks from a device cursor, G =
// floor(64 / s^2) listed pixels per wave, one lane per sample); the walk is written out once more here and not shared through
// a template, so that the sixteen instantiations of the plain and the deep refine kernels keep the registers and the code they
// have.  A lane's sample is sample (k_r, k_i) of the (W s) x (H s) view: dcm as deep_pixel forms it, then the loop of
// deep_wide_kernel or, with a table, of deep_wide_bla_kernel, put together from the functions those kernels are made of -- so
// count and |z|^2 are the bits mbk_deep_xview_launch stores for that sample.  The step loop is an ordinary divergent loop inside
// `if (valid)`: a lane without a sample executes no step, no wave-uniform value is taken from a lane inside it, and the wave is
// whole again when the colours are summed across a group.
#pragma once

#include "mbk_adaptive.h"
#include "mbk_deep_wide_bla.h"

namespace mbk {

struct DeepWideAdaptiveRefineArgs {
    DeepWideBlaArgs b;       // b.v: the wide orbit, exp2 and the window (col0 .. nrows) of the (W s) x (H s) view that holds the
                             // band's fine samples (fill_deep_window); no outputs.  The table (ke, ab, levels, off) with kXbla only.
    uint32_t nc;             // the band's columns (a list entry is row * nc + col)
    const uint32_t *list;
    const uint32_t *len;     // DEVICE memory: the host never learns it
    uint32_t *cursor;        // the next chunk of the list to hand out (zeroed by the host before the launch)
    uint32_t *out;           // the band's first pixel in the image
    uint64_t out_pitch;
    ReduceSlot *stats;       // may be null: the fine samples are added to these partial results
    RenderPalette pal;
};

// One fine sample: deep_wide_kernel's loop (kXbla false; any M) or deep_wide_bla_kernel's (kXbla true; M >= 2).
template <bool kXbla>
__device__ __forceinline__ void deep_wide_adaptive_sample(const DeepWideAdaptiveRefineArgs &a, double dcr, double dci, int32_t &count,
                                                          double &mag)
{
    const DeepWideArgs &p = a.b.v;
    const int32_t exp2 = p.exp2;
    count = 0;
    mag = 0.0;
    if constexpr (kXbla) {
        double wr, wi;
        int32_t q;
        wide_norm(dcr, dci, exp2, wr, wi, q);
        BlaCursor<WideEntry, int32_t> c(p.orbit, p.z1, p.M, a.b.ke, kWideZeroExp);
        for (int32_t i = 1; i < p.mrd; ++i) {
            if (wide_bla_within(q, c.r0)) {
                uint32_t l;
                const uint32_t at = wide_bla_climb(a.b.ke, a.b.off, a.b.levels, c.M, c.m, i, p.mrd, q, &l);
                const WideBlaEntry e = a.b.ab[at];
                wide_bla_apply(e.ar, e.ai, e.ae, e.br, e.bi, e.be, dcr, dci, exp2, wr, wi, q);
                c.skip(l);
                i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
            } else {
                wide_step(c.cur.xr, c.cur.xi, c.cur.xe, dcr, dci, exp2, wr, wi, q);
                c.step();
            }
            double zr, zi, mg;
            int32_t t;
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
    } else {
        double wr, wi, zr, zi, mg;
        int32_t q, t;
        OrbitCursor<WideEntry> c(p.orbit, p.z1, p.M, wide_start(p.z1, p.M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg));
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
    }
}

template <int S, bool kXbla>
__global__ __launch_bounds__(256) void deep_wide_adaptive_refine_kernel(const DeepWideAdaptiveRefineArgs a)
{
    constexpr uint32_t S2 = (uint32_t)(S * S), G = 64u / S2;
    const DeepWideArgs &p = a.b.v;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = lane / S2, sub = lane - g * S2, sy = sub / (uint32_t)S, sx = sub - sy * (uint32_t)S;
    const uint32_t n = *a.len;   // wave-uniform
    const uint32_t groups = n / G + (n % G != 0u ? 1u : 0u);
    const uint32_t chunks = gridDim.x * 4u * kAdaptiveChunksPerWave;
    const uint32_t per_chunk = groups / chunks + 1u;   // groups per request
    const unsigned long long cap = p.mrd > 1 ? (unsigned long long)p.mrd - 1ull : 0ull;
    unsigned long long iters = 0, never = 0;
    for (;;) {
        uint32_t chunk = 0u;
        if (lane == 0u) chunk = atomicAdd(a.cursor, 1u);
        chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
        const uint64_t first = (uint64_t)chunk * per_chunk;
        if (first >= (uint64_t)groups) break;
        const uint32_t last = (uint32_t)(first + per_chunk < (uint64_t)groups ? first + per_chunk : (uint64_t)groups);
        for (uint32_t grp = (uint32_t)first; grp < last; ++grp) {
            const uint64_t at = (uint64_t)grp * G + g;
            const bool valid = g < G && at < (uint64_t)n;
            uint32_t row = 0u, col = 0u, colour = 0u;
            if (valid) {
                const uint32_t idx = a.list[at];
                row = idx / a.nc;
                col = idx - row * a.nc;
                // dcm = fl(fl(k - (W s - 1) / 2) * step): deep_pixel's bits for sample (k_r, k_i) of the fine view
                const double dcr = ((double)(p.col0 + col * (uint32_t)S + sx) - p.half_r) * p.step_r;
                const double dci = ((double)(p.row0 + row * (uint32_t)S + sy) - p.half_i) * p.step_i;
                int32_t count;
                double mag;
                deep_wide_adaptive_sample<kXbla>(a, dcr, dci, count, mag);
                colour = render_colour_smooth(a.pal, a.pal.entries, count, smooth_value(count, mag));
                iters += count > 0 ? (unsigned long long)count : cap;
                never += count == 0 ? 1ull : 0ull;
            }
            // every lane of the wave is here again
            RenderSum sum;
            sum.even = adaptive_group_sum<S2>(render_even(colour), g * S2);
            sum.odd = adaptive_group_sum<S2>(render_odd(colour), g * S2);
            if (valid && sub == 0u) a.out[(uint64_t)row * a.out_pitch + col] = sum.mean(S2);
        }
    }
    if (a.stats) {
        iters = wave_sum_u64(iters);
        never = wave_sum_u64(never);
        if (lane == 0u) {
            ReduceOut *out = &a.stats[(blockIdx.x * 4u + (threadIdx.x >> 6)) % kReduceSlots].r;
            if (iters) atomicAdd(&out->pixel_iterations, iters);
            if (never) atomicAdd(&out->never_pixels, never);
        }
    }
}

template <bool kXbla>
inline void launch_deep_wide_adaptive_refine(uint32_t s, dim3 grid, hipStream_t stream, const DeepWideAdaptiveRefineArgs &a)
{
    const dim3 block(256);
    switch (s) {
        case 2: hipLaunchKernelGGL((deep_wide_adaptive_refine_kernel<2, kXbla>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((deep_wide_adaptive_refine_kernel<3, kXbla>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((deep_wide_adaptive_refine_kernel<4, kXbla>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((deep_wide_adaptive_refine_kernel<8, kXbla>), grid, block, 0, stream, a); break;
    }
}

}   // namespace mbk
