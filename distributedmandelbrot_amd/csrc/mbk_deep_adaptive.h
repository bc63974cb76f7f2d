// mbk_deep_adaptive.h -- adaptive supersampling of deep-view smooth renders (include/mbk.h, "Adaptive supersampling of deep
// views"): the refine kernel.  The base pass is the deep sample launch and the classify kernel is mbk_adaptive.h's, which works
// on samples and does not care what kind of view made them; what a deep view needs of its own is the kernel that computes the
// s x s fine samples of the listed pixels by perturbation.
//
// The list is walked as adaptive_refine_kernel walks it (a grid sized to the chip, chunks from a device cursor, G =
// floor(64 / s^2) listed pixels per wave, one lane per sample); the walk is written out a second time here and not shared
// through a template, so that the plain kernel's eight instantiations keep the registers and the code they have.  A lane's
// sample is sample (k_r, k_i) of the (W s) x (H s) view: dc as deep_pixel forms it, then the loop of deep_view_kernel or, with a
// table, of deep_bla_kernel, put together from the functions those kernels are made of -- so count and |z|^2 are the bits
// mbk_deep_view_launch stores for that sample.  The step loop is an ordinary divergent loop inside `if (valid)`: a lane
// without a sample executes no step, no wave-uniform value is taken from a lane inside it, and the wave is whole again when
// the colours are summed across a group.
#pragma once

#include "mbk_adaptive.h"
#include "mbk_deep_bla.h"

namespace mbk {

struct DeepAdaptiveRefineArgs {
    DeepBlaArgs b;           // b.v: the orbit and the window (col0 .. nrows) of the (W s) x (H s) view that holds the band's
                             // fine samples (fill_deep_window); no outputs.  The table (rc, ab, levels, off) with kBla only.
    uint32_t nc;             // the band's columns (a list entry is row * nc + col)
    const uint32_t *list;
    const uint32_t *len;     // DEVICE memory: the host never learns it
    uint32_t *cursor;        // the next chunk of the list to hand out (zeroed by the host before the launch)
    uint32_t *out;           // the band's first pixel in the image
    uint64_t out_pitch;
    ReduceSlot *stats;       // may be null: the fine samples are added to these partial results
    RenderPalette pal;
};

// One fine sample: deep_view_kernel's loop (kBla false; any M) or deep_bla_kernel's (kBla true; M >= 2).
template <bool kBla>
__device__ __forceinline__ void deep_adaptive_sample(const DeepAdaptiveRefineArgs &q, double dcr, double dci, int32_t &count, double &mag)
{
    const DeepArgs &p = q.b.v;
    count = 0;
    mag = 0.0;
    if constexpr (kBla) {
        double dzr = dcr, dzi = dci;
        BlaCursor<double4, double> c(p.orbit, p.z1, p.M, q.b.rc, 0.0);
        for (int32_t i = 1; i < p.mrd; ++i) {
            double ad;
            if (bla_within(dzr, dzi, c.r0, &ad)) {
                const uint32_t l = bla_climb(q.b.rc, q.b.off, q.b.levels, c.M, c.m, i, p.mrd, ad);
                const double4 e = q.b.ab[q.b.off[l] + ((c.m - 1u) >> l)];
                bla_apply(e.x, e.y, e.z, e.w, dcr, dci, dzr, dzi);
                c.skip(l);
                i += (int32_t)((1u << l) - 1u);
            } else {
                deep_plain_step(c.cur.z, c.cur.w, dcr, dci, dzr, dzi);
                c.step();
            }
            const double zr = c.nz.x + dzr, zi = c.nz.y + dzi;
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
    } else {
        double dzr, dzi, zr, zi;
        OrbitCursor<double4> c(p.orbit, p.z1, p.M, deep_start(p.z1.x, p.z1.y, p.M, dcr, dci, dzr, dzi, zr, zi));
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
    }
}

template <int S, bool kBla>
__global__ __launch_bounds__(256) void deep_adaptive_refine_kernel(const DeepAdaptiveRefineArgs q)
{
    constexpr uint32_t S2 = (uint32_t)(S * S), G = 64u / S2;
    const DeepArgs &p = q.b.v;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = lane / S2, sub = lane - g * S2, sy = sub / (uint32_t)S, sx = sub - sy * (uint32_t)S;
    const uint32_t n = *q.len;   // wave-uniform
    const uint32_t groups = n / G + (n % G != 0u ? 1u : 0u);
    const uint32_t chunks = gridDim.x * 4u * kAdaptiveChunksPerWave;
    const uint32_t per_chunk = groups / chunks + 1u;   // groups per request
    const unsigned long long cap = p.mrd > 1 ? (unsigned long long)p.mrd - 1ull : 0ull;
    unsigned long long iters = 0, never = 0;
    for (;;) {
        uint32_t chunk = 0u;
        if (lane == 0u) chunk = atomicAdd(q.cursor, 1u);
        chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
        const uint64_t first = (uint64_t)chunk * per_chunk;
        if (first >= (uint64_t)groups) break;
        const uint32_t last = (uint32_t)(first + per_chunk < (uint64_t)groups ? first + per_chunk : (uint64_t)groups);
        for (uint32_t grp = (uint32_t)first; grp < last; ++grp) {
            const uint64_t at = (uint64_t)grp * G + g;
            const bool valid = g < G && at < (uint64_t)n;
            uint32_t row = 0u, col = 0u, colour = 0u;
            if (valid) {
                const uint32_t idx = q.list[at];
                row = idx / q.nc;
                col = idx - row * q.nc;
                // dc = fl(fl(k - (W s - 1) / 2) * step): deep_pixel's bits for sample (k_r, k_i) of the fine view
                const double dcr = ((double)(p.col0 + col * (uint32_t)S + sx) - p.half_r) * p.step_r;
                const double dci = ((double)(p.row0 + row * (uint32_t)S + sy) - p.half_i) * p.step_i;
                int32_t count;
                double mag;
                deep_adaptive_sample<kBla>(q, dcr, dci, count, mag);
                colour = render_colour_smooth(q.pal, q.pal.entries, count, smooth_value(count, mag));
                iters += count > 0 ? (unsigned long long)count : cap;
                never += count == 0 ? 1ull : 0ull;
            }
            // every lane of the wave is here again
            RenderSum sum;
            sum.even = adaptive_group_sum<S2>(render_even(colour), g * S2);
            sum.odd = adaptive_group_sum<S2>(render_odd(colour), g * S2);
            if (valid && sub == 0u) q.out[(uint64_t)row * q.out_pitch + col] = sum.mean(S2);
        }
    }
    if (q.stats) {
        iters = wave_sum_u64(iters);
        never = wave_sum_u64(never);
        if (lane == 0u) {
            ReduceOut *out = &q.stats[(blockIdx.x * 4u + (threadIdx.x >> 6)) % kReduceSlots].r;
            if (iters) atomicAdd(&out->pixel_iterations, iters);
            if (never) atomicAdd(&out->never_pixels, never);
        }
    }
}

template <bool kBla>
inline void launch_deep_adaptive_refine(uint32_t s, dim3 grid, hipStream_t stream, const DeepAdaptiveRefineArgs &a)
{
    const dim3 block(256);
    switch (s) {
        case 2: hipLaunchKernelGGL((deep_adaptive_refine_kernel<2, kBla>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((deep_adaptive_refine_kernel<3, kBla>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((deep_adaptive_refine_kernel<4, kBla>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((deep_adaptive_refine_kernel<8, kBla>), grid, block, 0, stream, a); break;
    }
}

}   // namespace mbk
