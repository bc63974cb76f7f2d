// mbk_adaptive.h -- adaptive supersampling of plain-view smooth renders (include/mbk.h, "Adaptive supersampling"): the s x s
// samples are computed only for the output pixels whose s = 1 colour differs from a neighbour's by `threshold` or more.
//
// The difference and the decision are written once as __host__ __device__ functions, which the classify kernel and
// mbk_render_adaptive_host share with render_colour_smooth and RenderSum (mbk_render.h).  Per band three steps run on the
// stream: the base pass (the existing escape kernels on the band grown by one pixel and clamped to the VIEW), the classify
// kernel (colour, base image, mask, list of refined pixels) and the refine kernel (the fine samples of the listed pixels, one
// lane per sample, on the hand-scheduled loops seeded per lane as mbk_julia.h seeds them).  The length of the list never
// reaches the host.
//
// The refine kernels of all kinds of view are adaptive_walk around a sampler (here the plain view's; mbk_deep_adaptive.h,
// mbk_deep_wide_adaptive.h).  The sampler contract: the walk calls sample(valid, row, col, sx, sy) once per group of the list
// with EVERY lane of the wave present -- `valid` says whether the lane holds sample (sx, sy) of the listed pixel (row, col) of
// the band -- and takes back that sample's count and |z|^2.  A sampler may therefore take wave-level decisions (ballots, a
// grouped bailout test) at its top level, and must then give its lanes without a sample something harmless to run; whatever it
// runs under `if (valid)` is an ordinary divergent loop from which no wave-uniform value may be taken.  What it returns for
// an invalid lane is ignored.  The colour, the sums across a group (whole wave again) and the statistics are the walk's.
#pragma once

#include <vector>

#include "mbk_kernels.h"
#include "mbk_render.h"

namespace mbk {

// The per-channel maxima of |p.ch - q.ch| over the pairs added, two channels to a word as RenderSum holds them: the 16-bit
// halves are subtracted, made positive and folded in by packed instructions, so that a pixel's eight neighbours cost eight
// such steps and ONE comparison with the threshold.
typedef short AdaptivePair __attribute__((ext_vector_type(2)));
struct AdaptiveMax {
    AdaptivePair even = {0, 0}, odd = {0, 0};
    __host__ __device__ inline void add(uint32_t p, uint32_t q)
    {
        const AdaptivePair de = __builtin_bit_cast(AdaptivePair, render_even(p)) - __builtin_bit_cast(AdaptivePair, render_even(q));
        const AdaptivePair dn = __builtin_bit_cast(AdaptivePair, render_odd(p)) - __builtin_bit_cast(AdaptivePair, render_odd(q));
        even = __builtin_elementwise_max(even, __builtin_elementwise_max(de, -de));
        odd = __builtin_elementwise_max(odd, __builtin_elementwise_max(dn, -dn));
    }
    __host__ __device__ inline uint32_t max() const
    {
        const AdaptivePair m = __builtin_elementwise_max(even, odd);
        return (uint32_t)(m.x > m.y ? m.x : m.y);
    }
};

// diff(p, q): max over the four channels, alpha included, of |p.ch - q.ch|
__host__ __device__ inline uint32_t adaptive_diff(uint32_t p, uint32_t q)
{
    AdaptiveMax m;
    m.add(p, q);
    return m.max();
}

// Is pixel (x, y) of a w x h rectangle of base colours refined: does some neighbour's diff reach the threshold?  at(x, y): the
// colour of a pixel of the rectangle.  The neighbourhood is clamped at the rectangle's edges: the caller hands in the whole
// view, or a piece of it that holds every neighbour the view has (a band's halo).  threshold 0 refines everything -- a pixel
// without neighbours too --, 256 nothing (a difference is at most 255).
template <typename At>
__host__ __device__ inline bool adaptive_refined(uint32_t threshold, uint32_t x, uint32_t y, uint32_t w, uint32_t h, At at)
{
    if (threshold == 0u) return true;
    const uint32_t b = at(x, y);
    AdaptiveMax m;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t nx = x + (uint32_t)dx, ny = y + (uint32_t)dy;   // (x - 1 of x = 0 wraps to 2^32 - 1 >= w)
            if ((dx | dy) != 0 && nx < w && ny < h) m.add(b, at(nx, ny));
        }
    return m.max() >= threshold;
}

// The contract on the host for caller-supplied samples: base of the FULL width x height view, fine of the FULL
// (width s) x (height s) view.  mask may be null.
inline void render_adaptive_host(const RenderPalette &pal, uint32_t s, uint32_t threshold, uint32_t width, uint32_t height,
                                 const int32_t *base_counts, const double *base_smooth, const int32_t *fine_counts,
                                 const double *fine_smooth, uint8_t *rgba, uint8_t *mask)
{
    std::vector<uint32_t> base((size_t)width * height);
    for (size_t k = 0; k < base.size(); ++k) base[k] = render_colour_smooth(pal, pal.entries, base_counts[k], base_smooth[k]);
    const uint64_t pitch = (uint64_t)width * s;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const bool refined = adaptive_refined(threshold, x, y, width, height,
                                                  [&](uint32_t px, uint32_t py) { return base[(size_t)py * width + px]; });
            uint32_t c = base[(size_t)y * width + x];
            if (refined) {
                RenderSum sum;
                for (uint32_t sy = 0; sy < s; ++sy)
                    for (uint32_t sx = 0; sx < s; ++sx) {
                        const uint64_t at = ((uint64_t)y * s + sy) * pitch + (uint64_t)x * s + sx;
                        sum.add(render_colour_smooth(pal, pal.entries, fine_counts[at], fine_smooth[at]));
                    }
                c = sum.mean(s * s);
            }
            uint8_t *o = rgba + ((uint64_t)y * width + x) * 4u;
            o[0] = (uint8_t)c;
            o[1] = (uint8_t)(c >> 8);
            o[2] = (uint8_t)(c >> 16);
            o[3] = (uint8_t)(c >> 24);
            if (mask) mask[(size_t)y * width + x] = refined ? 1u : 0u;
        }
}

// ---- classify: a band's haloed base samples to base image, mask and list -------------------------------------------

constexpr uint32_t kAdaptiveTileX = 32, kAdaptiveTileY = 8;   // output pixels of a workgroup's tile: one lane each
constexpr uint32_t kAdaptiveCellsX = kAdaptiveTileX + 2u, kAdaptiveCells = kAdaptiveCellsX * (kAdaptiveTileY + 2u);

struct AdaptiveClassifyArgs {
    const int32_t *counts;   // the base samples of the halo rectangle, row pitch hc
    const double *smooth;
    uint32_t hc, hr;         // the halo rectangle: the band grown by one pixel and clamped to the view
    uint32_t ox, oy;         // the band's first pixel inside it (0 where the band touches the view's edge, else 1)
    uint32_t nc, nr;         // the band
    uint32_t tiles_x;
    uint32_t threshold;
    uint32_t mrd;
    uint32_t lds_palette;    // the palette is staged in (dynamic) LDS
    uint32_t *out;           // the band's first pixel in the image, row pitch out_pitch words
    uint8_t *mask;           // may be null: the band's first pixel in the mask, row pitch out_pitch bytes
    uint64_t out_pitch;
    uint32_t *list;          // the refined pixels' band indices row * nc + col, in any order
    uint32_t *len;           // their number (zeroed by the host before the launch)
    ReduceSlot *stats;       // may be null: the band's own base samples are added to these partial results
    RenderPalette pal;
};

// A workgroup takes 32 x 8 tiles of the band in turn.  The 34 x 10 colours around a tile are evaluated once and staged in LDS,
// then every lane compares its pixel's word with up to eight others: 1.33 colour evaluations per pixel where comparing on the
// fly costs nine.  Streaming: 12 bytes in, 4 (+ 1) out per pixel; a refined pixel costs its wave one share of a ballot and of
// one atomic reservation in the list.
__global__ __launch_bounds__(256) void adaptive_classify_kernel(const AdaptiveClassifyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_adaptive_palette[];
    __shared__ uint32_t s_tile[kAdaptiveCells];
    const uint32_t *entries = a.pal.entries;
    if (a.lds_palette) {
        for (uint32_t k = threadIdx.x; k < a.pal.n; k += 256u) s_adaptive_palette[k] = a.pal.entries[k];
        entries = s_adaptive_palette;
    }
    const uint32_t lx = threadIdx.x & (kAdaptiveTileX - 1u), ly = threadIdx.x / kAdaptiveTileX;
    const uint32_t tiles = a.tiles_x * ((a.nr + kAdaptiveTileY - 1u) / kAdaptiveTileY);
    const unsigned long long cap = a.mrd > 1u ? (unsigned long long)a.mrd - 1ull : 0ull;
    unsigned long long iters = 0, never = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        // the halo coordinates of tile cell (0, 0), which is one pixel up and left of the tile: may be "-1" (wraps)
        const uint32_t hx0 = tx * kAdaptiveTileX + a.ox - 1u, hy0 = ty * kAdaptiveTileY + a.oy - 1u;
        __syncthreads();   // the palette is in place; the previous tile has been read
        for (uint32_t k = threadIdx.x; k < kAdaptiveCells; k += 256u) {
            const uint32_t cy = k / kAdaptiveCellsX, cx = k - cy * kAdaptiveCellsX;
            const uint32_t hx = hx0 + cx, hy = hy0 + cy;
            if (hx < a.hc && hy < a.hr) {
                const uint64_t at = (uint64_t)hy * a.hc + hx;
                s_tile[k] = render_colour_smooth(a.pal, entries, a.counts[at], a.smooth[at]);
            }
        }
        __syncthreads();
        const uint32_t col = tx * kAdaptiveTileX + lx, row = ty * kAdaptiveTileY + ly;
        bool refined = false;
        if (col < a.nc && row < a.nr) {
            const uint32_t hx = col + a.ox, hy = row + a.oy;
            refined = adaptive_refined(a.threshold, hx, hy, a.hc, a.hr, [&](uint32_t px, uint32_t py) {
                return s_tile[(py - hy0) * kAdaptiveCellsX + (px - hx0)];
            });
            a.out[(uint64_t)row * a.out_pitch + col] = s_tile[(ly + 1u) * kAdaptiveCellsX + lx + 1u];
            if (a.mask) a.mask[(uint64_t)row * a.out_pitch + col] = refined ? 1u : 0u;
            if (a.stats) {
                const int32_t c = a.counts[(uint64_t)hy * a.hc + hx];
                iters += c > 0 ? (unsigned long long)c : cap;
                never += c == 0 ? 1ull : 0ull;
            }
        }
        // one reservation per wave: the lanes of the ballot take consecutive entries
        const unsigned long long votes = __ballot(refined);
        if (votes != 0ull) {
            const uint32_t lane = threadIdx.x & 63u;
            const uint32_t leader = (uint32_t)__builtin_ctzll(votes);
            uint32_t first = 0u;
            if (lane == leader) first = atomicAdd(a.len, (uint32_t)__builtin_popcountll(votes));
            first = (uint32_t)__shfl((int)first, (int)leader, 64);
            if (refined) a.list[first + (uint32_t)__builtin_popcountll(votes & ((1ull << lane) - 1ull))] = row * a.nc + col;
        }
    }
    if (a.stats) {
        iters = wave_sum_u64(iters);
        never = wave_sum_u64(never);
        if ((threadIdx.x & 63u) == 0u) {
            ReduceOut *out = &a.stats[blockIdx.x % kReduceSlots].r;
            if (iters) atomicAdd(&out->pixel_iterations, iters);
            if (never) atomicAdd(&out->never_pixels, never);
        }
    }
}

// ---- refine: the s x s samples of the listed pixels ------------------------------------------------------------------

// What the walk of the list needs, whatever the kind of view: the refine kernels' arguments all embed it.
struct AdaptiveWalkArgs {
    uint32_t nc;             // the band's columns (a list entry is row * nc + col)
    const uint32_t *list;
    const uint32_t *len;     // DEVICE memory: the host never learns it
    uint32_t *cursor;        // the next chunk of the list to hand out (zeroed by the host before the launch)
    uint32_t *out;           // the band's first pixel in the image
    uint64_t out_pitch;
    ReduceSlot *stats;       // may be null: the fine samples are added to these partial results
    RenderPalette pal;
};

// The sum of v over the S2 lanes of the caller's group (lanes g S2 .. g S2 + S2 - 1), in every lane of it.  Powers of two
// fold with a butterfly that never leaves the aligned group; 9 does not align and reads its lanes one by one.
template <uint32_t S2>
__device__ __forceinline__ uint32_t adaptive_group_sum(uint32_t v, uint32_t first_lane)
{
    if constexpr ((S2 & (S2 - 1u)) == 0u) {
#pragma unroll
        for (uint32_t off = 1u; off < S2; off <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)off, 64);
        return v;
    } else {
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t k = 0u; k < S2; ++k) sum += (uint32_t)__shfl((int)v, (int)((first_lane + k) & 63u), 64);
        return sum;
    }
}

// Chunks of the list a wave takes over the launch, on average: what it asks of the cursor.  One request per group would be
// 16.7 M atomics on one address for a 4096^2 image at s = 8 and threshold 0; a handful per wave keeps the shares of the work
// within a fraction of a wave's run of each other (a refined pixel on the set's boundary costs up to mrd - 1 steps, one in the
// exterior a few: equal shares of the list would not be equal shares of the work).
constexpr uint32_t kAdaptiveChunksPerWave = 4;

// The walk of a refine kernel (256-thread workgroups), for supersampling S and mrd the view's: a grid sized to the chip; every
// wave takes chunks of the list from a cursor until the list is exhausted, and walks a chunk in groups of G = floor(64 / s^2)
// listed pixels, one lane per sample.  Per group every lane calls the sampler (the contract is at the top of this file); the
// walk colours the samples, sums the colours across a group with the whole wave present, stores the mean and adds the samples
// to the statistics.  Lanes without a sample (the 64th at s = 3, a part-filled last group) add colour 0 and store nothing.
template <int S, typename Sampler>
__device__ __forceinline__ void adaptive_walk(const AdaptiveWalkArgs &w, int32_t mrd, Sampler sample)
{
    constexpr uint32_t S2 = (uint32_t)(S * S), G = 64u / S2;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = lane / S2, sub = lane - g * S2, sy = sub / (uint32_t)S, sx = sub - sy * (uint32_t)S;
    const uint32_t n = *w.len;   // wave-uniform
    const uint32_t groups = n / G + (n % G != 0u ? 1u : 0u);
    const uint32_t chunks = gridDim.x * 4u * kAdaptiveChunksPerWave;
    const uint32_t per_chunk = groups / chunks + 1u;   // groups per request
    const unsigned long long cap = mrd > 1 ? (unsigned long long)mrd - 1ull : 0ull;
    unsigned long long iters = 0, never = 0;
    for (;;) {
        uint32_t chunk = 0u;
        if (lane == 0u) chunk = atomicAdd(w.cursor, 1u);
        chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk);
        const uint64_t first = (uint64_t)chunk * per_chunk;
        if (first >= (uint64_t)groups) break;
        const uint32_t last = (uint32_t)(first + per_chunk < (uint64_t)groups ? first + per_chunk : (uint64_t)groups);
        for (uint32_t grp = (uint32_t)first; grp < last; ++grp) {
            const uint64_t at = (uint64_t)grp * G + g;
            const bool valid = g < G && at < (uint64_t)n;
            uint32_t row = 0u, col = 0u;
            if (valid) {
                const uint32_t idx = w.list[at];
                row = idx / w.nc;
                col = idx - row * w.nc;
            }
            const EscapeSample f = sample(valid, row, col, sx, sy);
            const uint32_t colour = valid ? render_colour_smooth(w.pal, w.pal.entries, f.count, smooth_value(f.count, f.mag)) : 0u;
            // every lane of the wave is here
            RenderSum sum;
            sum.even = adaptive_group_sum<S2>(render_even(colour), g * S2);
            sum.odd = adaptive_group_sum<S2>(render_odd(colour), g * S2);
            if (valid) {
                if (sub == 0u) w.out[(uint64_t)row * w.out_pitch + col] = sum.mean(S2);
                iters += f.count > 0 ? (unsigned long long)f.count : cap;
                never += f.count == 0 ? 1ull : 0ull;
            }
        }
    }
    if (w.stats) {
        iters = wave_sum_u64(iters);
        never = wave_sum_u64(never);
        if (lane == 0u) {
            ReduceOut *out = &w.stats[(blockIdx.x * 4u + (threadIdx.x >> 6)) % kReduceSlots].r;
            if (iters) atomicAdd(&out->pixel_iterations, iters);
            if (never) atomicAdd(&out->never_pixels, never);
        }
    }
}

// Family: the refine kernels of a kind of view -- Args, and kernel<S> the instantiation for supersampling S
template <typename Family>
inline void launch_adaptive_refine(uint32_t s, dim3 grid, hipStream_t stream, const typename Family::Args &a)
{
    const dim3 block(256);
    switch (s) {
        case 2: hipLaunchKernelGGL((Family::template kernel<2>), grid, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((Family::template kernel<3>), grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((Family::template kernel<4>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((Family::template kernel<8>), grid, block, 0, stream, a); break;
    }
}

// ---- the plain view's refine kernel ----------------------------------------------------------------------------------------

struct AdaptiveRefineArgs {
    AdaptiveWalkArgs w;
    Axis re, im;             // the axes of the (W s) x (H s) view
    uint32_t px0, py0;       // the band's first pixel in the W x H view
    int32_t mrd;
    uint32_t exact_steps;    // the grouped loop: steps tested one by one first; its cycle test's window (as TileArgs)
    uint32_t cyc_window;
};

// The count and |z|^2 of a sample are the bits the tile kernels store for it (block_pixel): the coordinates are axis_value's, a
// wave that holds a non-zero |c_i| below 2^-900 takes the literal doubling (for every other c_i both doublings round alike,
// kSafeImagMin), and a wave within 1e-9 of the ring |c| = 2 takes the per-step test.  kGroup = 0: the per-step loop throughout;
// 8: 8-step groups with the cycle test, which retires the samples inside the set early and yields the same counts.  These
// three decisions are the wave's, taken with every lane present; lanes without a sample run c = 4, which leaves at step 1.
template <int S, int kGroup>
__global__ __launch_bounds__(256) void adaptive_refine_kernel(const AdaptiveRefineArgs p)
{
    adaptive_walk<S>(p.w, p.mrd, [&p](bool valid, uint32_t row, uint32_t col, uint32_t sx, uint32_t sy) {
        double cr = 4.0, ci = 0.0;
        if (valid) {
            cr = axis_value(p.re, (p.px0 + col) * (uint32_t)S + sx);
            ci = axis_value(p.im, (p.py0 + row) * (uint32_t)S + sy);
        }
        double m = 0.0;
        int32_t count;
        const bool literal = __ballot(ci != 0.0 && __builtin_fabs(ci) < kSafeImagMin) != 0ull;
        if (literal)
            count = escape_count_asm_from<false>(cr, ci, cr, ci, p.mrd, &m);
        else if (kGroup == 0 || wave_touches_ring(cr, ci))
            count = escape_count_asm_from<true>(cr, ci, cr, ci, p.mrd, &m);
        else
            count = escape_count_group_from<8, true>(cr, ci, cr, ci, p.mrd, &m, p.exact_steps, p.cyc_window);
        return EscapeSample{count, m};
    });
}

template <int kGroup>
struct AdaptiveRefine {
    using Args = AdaptiveRefineArgs;
    template <int S>
    static constexpr auto kernel = adaptive_refine_kernel<S, kGroup>;
};

}   // namespace mbk
