// mbk_density.h -- Buddhabrot density views (include/mbk.h, "Density views"): the orbits of the escaping samples of a view,
// replayed and accumulated into a 2-D table of 32-bit cells, plus what a caller needs to look at such a table: its maximum
// and total, and a resolve that sends it through a palette.  The cell rule, the replay step and the colour of a cell are
// written once as __host__ __device__ functions that the kernels and the host twins (mbk_density_*_host) share.
//
// Two passes, like the default distance path (mbk_distance.h): the escape kernels write the window's counts, cycle test and
// all -- for a density view the interior is pure waste, and they retire it for nearly nothing --, then the replay kernel runs
// each qualifying sample for exactly its n steps with no bailout test and issues one 32-bit global atomic add without a
// return value (global_atomic_add_u32) per orbit point that lands inside the target.  Integer sums: the table is exact
// whatever the schedule.
//
// Arithmetic (the translation unit is compiled with -ffp-contract=off: every operation below rounds on its own):
//   step   zr' = fl(fl(fl(zr zr) - fl(zi zi)) + cr),  zi' = fl(fl(fl(2 zr) zi) + ci)     the reference's literal form
//   cell   tx = fl(fl(zr - start_r) inv_r), ty likewise; inside iff 0 <= tx < W and 0 <= ty < H (false for NaN); the cell is
//          (trunc tx, trunc ty), which is the floor for tx >= 0 (and 0 for -0.0)
// Per step 7 fp64 VALU for z, 4 for the cell, two conversions, four compares, the address and the atomic.  The replay uses the
// literal doubling everywhere: it equals the count kernels' fused form wherever they are allowed to use it, and needs no
// host-side rule.
//
// The replay is built two ways (MBK_DENSITY_COMPACT, a compile-time switch: profiles/density/README.md has the A/B):
//   plain    one lane per sample in image order, 8x8 blocks, single-wave workgroups (the distance kernel's shape).  A block
//            without a qualifying sample ends after one load; the step counter is wave-uniform and a lane leaves by an integer
//            compare against its own n.  Neighbouring samples have neighbouring orbits for their first steps, so a wave's
//            atomics start out on neighbouring cells.
//   compact  the qualifying samples are first listed, ordered by count band (floor(log2 n), long orbits first) with a
//            counting pass and a scatter pass (LDS counters per workgroup, one global atomic per band and workgroup); the
//            replay then takes 64 list entries to a wave, whose lanes run within a factor of two of each other.
//
// Nothing is written outside the W x H words: a cell index is formed only from 0 <= tx < W, 0 <= ty < H.
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mbk_kernels.h"
#include "mbk_render.h"

#ifndef MBK_DENSITY_COMPACT
#define MBK_DENSITY_COMPACT 0
#endif

namespace mbk {

constexpr bool kDensityCompact = MBK_DENSITY_COMPACT != 0;
constexpr uint32_t kDensityBands = 32;        // count bands of the compacted list: floor(log2 n), n < 2^31
constexpr uint32_t kDensityThreads = 256;     // list building, maximum, resolve

// The target as the kernels see it: inv_* = fl(W / range_r), fl(H / range_i), computed once on the host.
struct DensityTarget {
    double start_r, start_i;
    double inv_r, inv_i;
    double w, h;              // (double)width, (double)height
    uint32_t width, height;
};

// The cell of one point, or false (outside, NaN).
__host__ __device__ inline bool density_cell(const DensityTarget &t, double zr, double zi, uint32_t *cx, uint32_t *cy)
{
    const double dx = zr - t.start_r;
    const double tx = dx * t.inv_r;
    const double dy = zi - t.start_i;
    const double ty = dy * t.inv_i;
    if (!(tx >= 0.0 && tx < t.w && ty >= 0.0 && ty < t.h)) return false;
    *cx = (uint32_t)tx;   // 0 <= tx < 2^28: the conversion truncates, which is the floor
    *cy = (uint32_t)ty;
    return true;
}

// One step of the orbit, the literal form.
__host__ __device__ inline void density_step(double &zr, double &zi, double cr, double ci)
{
    const double a = zr * zr, b = zi * zi;
    const double t = a - b;
    const double w = 2.0 * zr;
    const double q = w * zi;
    zr = t + cr;
    zi = q + ci;
}

struct DensityArgs {
    Axis re, im;
    uint32_t col0, row0, ncols, nrows;
    uint32_t blocks_x;            // plain: 8x8 blocks per block row (1-D grid, row-major)
    int32_t min_count, max_count; // a sample qualifies when min_count <= n <= max_count (1 <= min_count)
    DensityTarget t;
    const int32_t *counts;        // the window's counts (window layout)
    uint32_t *table;              // height x width cells
    unsigned long long *stat;     // may be null: [0] += deposits, [1] += points dropped
    // compact: the list of qualifying samples (window offsets), the band totals [0 .. 32) and the band cursors [32 .. 64)
    uint32_t *list;
    uint32_t *bands;
};

__device__ __forceinline__ int32_t density_qualify(const DensityArgs &p, int32_t n)
{
    return (n >= p.min_count && n <= p.max_count) ? n : 0;
}

// The orbit points z_0 .. z_(n-1) of one lane; nmax: the largest n of the wave (uniform).  Returns the lane's deposits.
__device__ __forceinline__ uint32_t density_replay(const DensityArgs &p, double cr, double ci, int32_t n, int32_t nmax)
{
    double zr = cr, zi = ci;
    uint32_t dep = 0u;
    for (int32_t k = 0; k < nmax; ++k) {
        if (k < n) {
            uint32_t cx, cy;
            if (density_cell(p.t, zr, zi, &cx, &cy)) {
                atomicAdd(&p.table[cy * p.t.width + cx], 1u);   // (W H <= 2^28: the index fits 32 bits)
                ++dep;
            }
            density_step(zr, zi, cr, ci);
        }
    }
    return dep;
}

__device__ __forceinline__ int32_t density_wave_max(int32_t n)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t other = __shfl_xor(n, off);
        n = other > n ? other : n;
    }
    return __builtin_amdgcn_readfirstlane(n);
}

// deposits and dropped points of a wave: two 64-bit atomics per wave that deposited anything
__device__ __forceinline__ void density_wave_stat(unsigned long long *stat, uint32_t dep, int32_t n, uint32_t lane)
{
    unsigned long long d = dep, all = (unsigned long long)(uint32_t)n;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        d += __shfl_xor(d, off);
        all += __shfl_xor(all, off);
    }
    if (lane == 0u && all) {
        atomicAdd(&stat[0], d);
        atomicAdd(&stat[1], all - d);
    }
}

// plain: one lane per sample, image order
__global__ __launch_bounds__(64) void density_replay_kernel(const DensityArgs p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    const uint32_t lc = bx * 8u + (lane & 7u), lr = by * 8u + (lane >> 3);
    const bool live = lc < p.ncols && lr < p.nrows;
    int32_t n = live ? density_qualify(p, p.counts[(size_t)lr * p.ncols + lc]) : 0;
    if (__ballot(n > 0) == 0ull) return;   // nothing qualifies: the interior, the far exterior under min_count
    const double cr = axis_value(p.re, p.col0 + (live ? lc : 0u));
    const double ci = axis_value(p.im, p.row0 + (live ? lr : 0u));
    const uint32_t dep = density_replay(p, cr, ci, n, density_wave_max(n));
    if (p.stat) density_wave_stat(p.stat, dep, n, lane);
}

// compact, pass 1: the number of qualifying samples per count band
__global__ __launch_bounds__(kDensityThreads) void density_band_count_kernel(const DensityArgs p)
{
    __shared__ uint32_t s_cnt[kDensityBands];
    if (threadIdx.x < kDensityBands) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t px = (uint64_t)p.ncols * p.nrows;
    const uint64_t o = (uint64_t)blockIdx.x * kDensityThreads + threadIdx.x;
    const int32_t n = o < px ? density_qualify(p, p.counts[o]) : 0;
    if (n > 0) atomicAdd(&s_cnt[31 - __clz(n)], 1u);
    __syncthreads();
    if (threadIdx.x < kDensityBands && s_cnt[threadIdx.x]) atomicAdd(&p.bands[threadIdx.x], s_cnt[threadIdx.x]);
}

// compact, pass 2: the list, band 30 first.  A band's part starts where the longer bands end; a workgroup reserves its share
// of each band with one returning atomic on the band's cursor.  list holds px entries at most: every sample is listed once.
__global__ __launch_bounds__(kDensityThreads) void density_band_scatter_kernel(const DensityArgs p)
{
    __shared__ uint32_t s_cnt[kDensityBands], s_base[kDensityBands];
    if (threadIdx.x < kDensityBands) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t px = (uint64_t)p.ncols * p.nrows;
    const uint64_t o = (uint64_t)blockIdx.x * kDensityThreads + threadIdx.x;
    const int32_t n = o < px ? density_qualify(p, p.counts[o]) : 0;
    const uint32_t band = n > 0 ? 31u - (uint32_t)__clz(n) : 0u;
    uint32_t rank = 0u;
    if (n > 0) rank = atomicAdd(&s_cnt[band], 1u);
    __syncthreads();
    if (threadIdx.x < kDensityBands && s_cnt[threadIdx.x]) {
        uint32_t start = 0u;
        for (uint32_t b = threadIdx.x + 1u; b < kDensityBands; ++b) start += p.bands[b];
        s_base[threadIdx.x] = start + atomicAdd(&p.bands[kDensityBands + threadIdx.x], s_cnt[threadIdx.x]);
    }
    __syncthreads();
    if (n > 0) p.list[s_base[band] + rank] = (uint32_t)o;
}

// compact, pass 3: 64 list entries to a wave.  The grid covers the whole window (the list's length is on the device); a wave
// beyond the list ends after one load.
__global__ __launch_bounds__(64) void density_replay_list_kernel(const DensityArgs p)
{
    const uint32_t lane = threadIdx.x;
    uint32_t total = 0u;
    for (uint32_t b = 0; b < kDensityBands; ++b) total += p.bands[b];
    const uint64_t at = (uint64_t)blockIdx.x * 64u + lane;
    if ((uint64_t)blockIdx.x * 64u >= total) return;
    const bool live = at < total;
    const uint32_t o = live ? p.list[at] : 0u;
    const int32_t n = live ? p.counts[o] : 0;   // (listed: it qualifies)
    const uint32_t lr = o / p.ncols, lc = o - lr * p.ncols;
    const double cr = axis_value(p.re, p.col0 + lc);
    const double ci = axis_value(p.im, p.row0 + lr);
    const uint32_t dep = density_replay(p, cr, ci, n, density_wave_max(n));
    if (p.stat) density_wave_stat(p.stat, dep, n, lane);
}

// Both passes over the counts of one window, on `stream`.  bands: 64 words the caller has cleared on the stream (compact).
inline void launch_density_replay(DensityArgs a, hipStream_t stream)
{
    const uint64_t px = (uint64_t)a.ncols * a.nrows;
    if (kDensityCompact) {
        const dim3 grid((uint32_t)((px + kDensityThreads - 1u) / kDensityThreads)), block(kDensityThreads);
        hipLaunchKernelGGL(density_band_count_kernel, grid, block, 0, stream, a);
        hipLaunchKernelGGL(density_band_scatter_kernel, grid, block, 0, stream, a);
        hipLaunchKernelGGL(density_replay_list_kernel, dim3((uint32_t)((px + 63u) / 64u)), dim3(64), 0, stream, a);
    } else {
        a.blocks_x = (a.ncols + 7u) / 8u;
        const dim3 grid(a.blocks_x * ((a.nrows + 7u) / 8u)), block(64);   // (at most 2^31 / 64 blocks: validate_view)
        hipLaunchKernelGGL(density_replay_kernel, grid, block, 0, stream, a);
    }
}

// The whole contract for one window on the host: mbk_density_accumulate_host.  counts: the window's counts.
inline void density_accumulate_host(const double *cr, const double *ci, uint32_t ncols, uint32_t nrows, const int32_t *counts,
                                    int32_t min_count, int32_t max_count, const DensityTarget &t, uint32_t *table,
                                    uint64_t *deposits, uint64_t *dropped)
{
    for (uint32_t r = 0; r < nrows; ++r)
        for (uint32_t c = 0; c < ncols; ++c) {
            const int32_t n = counts[(size_t)r * ncols + c];
            if (n < min_count || n > max_count) continue;
            double zr = cr[c], zi = ci[r];
            for (int32_t k = 0; k < n; ++k) {
                uint32_t cx, cy;
                if (density_cell(t, zr, zi, &cx, &cy)) {
                    ++table[(size_t)cy * t.width + cx];
                    ++*deposits;
                } else {
                    ++*dropped;
                }
                density_step(zr, zi, cr[c], ci[r]);
            }
        }
}

// ---- the maximum and the total of a table -------------------------------------------------------------------------------

struct DensityMax {
    unsigned long long total;
    uint32_t max, pad;
};

__global__ __launch_bounds__(kDensityThreads) void density_max_kernel(const uint32_t *table, uint64_t n, DensityMax *out)
{
    __shared__ unsigned long long s_total;
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) {
        s_total = 0ull;
        s_max = 0u;
    }
    __syncthreads();
    unsigned long long total = 0ull;
    uint32_t mx = 0u;
    for (uint64_t k = (uint64_t)blockIdx.x * kDensityThreads + threadIdx.x; k < n; k += (uint64_t)gridDim.x * kDensityThreads) {
        const uint32_t v = table[k];
        total += v;
        mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        total += __shfl_xor(total, off);
        const uint32_t other = (uint32_t)__shfl_xor((int)mx, off);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&s_total, total);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_total) {
        atomicAdd(&out->total, s_total);
        atomicMax(&out->max, s_max);
    }
}

// ---- a table as an image --------------------------------------------------------------------------------------------------

// The colour of one cell: g(v) = v or fl(sqrt(v)) (v < 2^32 is exact in binary64, the square root correctly rounded), then the
// MBK_RENDER_DISTANCE rule -- t = fl(fl(g scale) + offset), no wrap -- with g in place of de.  A cell is never `inside`.
__host__ __device__ inline uint32_t density_colour(const RenderPalette &p, const uint32_t *entries, bool root, uint32_t v)
{
    const double x = (double)v;
    return render_colour_distance(p, entries, 1, root ? sqrt(x) : x);
}

struct DensityResolveArgs {
    const uint32_t *table;   // height x width cells
    uint32_t *out;           // (height / k) x (width / k) pixels
    uint32_t width, out_w, out_h;
    uint32_t root;
    RenderPalette pal;
};

template <int K>
__global__ __launch_bounds__(kDensityThreads) void density_resolve_kernel(const DensityResolveArgs a)
{
    const uint64_t px = (uint64_t)a.out_w * a.out_h;
    for (uint64_t o = (uint64_t)blockIdx.x * kDensityThreads + threadIdx.x; o < px; o += (uint64_t)gridDim.x * kDensityThreads) {
        const uint32_t y = (uint32_t)(o / a.out_w), x = (uint32_t)(o - (uint64_t)y * a.out_w);
        RenderSum sum;
#pragma unroll
        for (int sy = 0; sy < K; ++sy)
#pragma unroll
            for (int sx = 0; sx < K; ++sx)
                sum.add(density_colour(a.pal, a.pal.entries, a.root != 0u, a.table[((uint64_t)y * K + sy) * a.width + (uint64_t)x * K + sx]));
        a.out[o] = sum.mean(K * K);
    }
}

inline void launch_density_resolve(uint32_t k, dim3 grid, hipStream_t stream, const DensityResolveArgs &a)
{
    const dim3 block(kDensityThreads);
    switch (k) {
        case 1: hipLaunchKernelGGL(density_resolve_kernel<1>, grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(density_resolve_kernel<2>, grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL(density_resolve_kernel<4>, grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL(density_resolve_kernel<8>, grid, block, 0, stream, a); break;
    }
}

inline void density_resolve_host(const RenderPalette &pal, bool root, uint32_t k, uint32_t width, uint32_t height,
                                 const uint32_t *table, uint8_t *rgba)
{
    const uint32_t ow = width / k, oh = height / k;
    for (uint32_t y = 0; y < oh; ++y)
        for (uint32_t x = 0; x < ow; ++x) {
            RenderSum sum;
            for (uint32_t sy = 0; sy < k; ++sy)
                for (uint32_t sx = 0; sx < k; ++sx)
                    sum.add(density_colour(pal, pal.entries, root, table[((uint64_t)y * k + sy) * width + (uint64_t)x * k + sx]));
            const uint32_t c = sum.mean(k * k);
            uint8_t *o = rgba + ((uint64_t)y * ow + x) * 4u;
            o[0] = (uint8_t)c;
            o[1] = (uint8_t)(c >> 8);
            o[2] = (uint8_t)(c >> 16);
            o[3] = (uint8_t)(c >> 24);
        }
}

}   // namespace mbk
