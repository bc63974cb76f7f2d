// mbk_chunks.h -- stored chunks (include/mbk.h, "Stored chunks"): the inverse of the on-device serialiser.  A chunk stream
// (code byte + Raw bytes or 5-byte RLE records) is validated and expanded on the device, and a decoded 4096 x 4096 chunk is
// coloured through a 256-entry palette and box-filtered by k in {1 .. 64} into an RGBA8 rectangle of a larger image.
//
// The rules live in __host__ __device__ functions (chunk_unpack4, chunk_status_of, chunk_mean) that the kernels and the
// host entry points (mbk_chunk_stream_check, mbk_chunk_decode_host, mbk_chunk_resolve_host) share.
//
// Device layout of an RLE payload: the bytes after the code byte, uploaded to a 256-byte aligned address, so that records
// 4 g .. 4 g + 3 are the five aligned dwords 5 g .. 5 g + 4.  A lane takes four records; a wave's loads are contiguous.
//
//   chunk_block_sums_kernel   1024 records per workgroup: 64-bit sum of the run lengths, "holds a zero run"
//   chunk_scan_sums_kernel    one workgroup: exclusive scan of the block sums, the total, and from them the reason code
//   chunk_starts_kernel       the run starts (exclusive prefix sum, clamped to n: a valid start is < 2^24) and values
//   chunk_expand_kernel       output-driven: a workgroup owns 4096 output bytes, finds the runs that cover them by binary
//                             search, stages their starts in LDS; a lane builds and stores 16 bytes
//   chunk_resolve_kernel      k <= 8: a lane owns four adjacent output pixels
//   chunk_resolve_split_kernel  k >= 16: a pixel is split over k / 16 lanes and four row parts and reduced
//   chunk_fill_kernel         a chunk of one value: the rectangle is palette[v]
// No atomics anywhere; every store is guarded by the bounds of the output, whatever the stream holds.
#pragma once

#include <cstdint>
#include <cstring>
#include <hip/hip_runtime.h>

#include "mbk_kernels.h"   // wave_sum_u64
#include "mbk_render.h"    // RenderSum

namespace mbk {

// reason codes: MBK_STREAM_* of include/mbk.h
constexpr uint32_t kStreamOk = 0, kStreamBadCodec = 1, kStreamBadSize = 2, kStreamZeroRun = 3, kStreamTooLong = 4,
                   kStreamTooShort = 5;

constexpr uint32_t kChunkDim = 4096;                 // MBK_CHUNK_DEFINITION
constexpr uint32_t kChunkScanThreads = 256;
constexpr uint32_t kChunkScanRecords = 4 * kChunkScanThreads;   // per workgroup
constexpr uint32_t kChunkPiece = 4096;               // output bytes a workgroup of the expansion owns (256 lanes x 16)
constexpr uint32_t kChunkPieceRuns = 4096;           // a valid stream starts at most this many runs inside a piece, + 1 before it

// Records 4 g .. 4 g + 3 from their five little-endian dwords: run lengths and the four values packed into one word.
__host__ __device__ inline void chunk_unpack4(const uint32_t (&w)[5], uint32_t (&len)[4], uint32_t &vals)
{
    len[0] = w[0];
    len[1] = (w[1] >> 8) | (w[2] << 24);
    len[2] = (w[2] >> 16) | (w[3] << 16);
    len[3] = (w[3] >> 24) | (w[4] << 8);
    vals = (w[1] & 0xffu) | (w[2] & 0xff00u) | (w[3] & 0xff0000u) | (w[4] & 0xff000000u);
}

// The reason code of an RLE payload from what the reductions yield.  A zero run wins over a wrong total (it does not
// depend on where in the stream either is found, so the device needs no order).
__host__ __device__ inline uint32_t chunk_status_of(bool zero_run, unsigned long long total, unsigned long long n)
{
    return zero_run ? kStreamZeroRun : (total > n ? kStreamTooLong : (total < n ? kStreamTooShort : kStreamOk));
}

// (2 S + k^2) / (2 k^2) rounded down, k = 2^lk: a shift.
__host__ __device__ inline uint32_t chunk_mean(uint32_t sum, uint32_t lk) { return (2u * sum + (1u << (2u * lk))) >> (1u + 2u * lk); }

__host__ __device__ inline uint32_t chunk_mean4(const uint32_t (&s)[4], uint32_t lk)
{
    return chunk_mean(s[0], lk) | (chunk_mean(s[1], lk) << 8) | (chunk_mean(s[2], lk) << 16) | (chunk_mean(s[3], lk) << 24);
}

// ---- host forms ------------------------------------------------------------------------------------------------------

// Walks the records of an RLE payload (`payload` = stream + 1, `runs` records): the reason code.
inline uint32_t chunk_check_records_host(const uint8_t *payload, uint64_t runs, uint64_t n)
{
    unsigned long long total = 0;
    bool zero = false;
    for (uint64_t g = 0; g < runs; g += 4) {
        uint8_t raw[20] = {};
        const uint64_t have = runs - g < 4 ? runs - g : 4;
        std::memcpy(raw, payload + 5 * g, 5 * have);
        uint32_t w[5], len[4], vals;
        for (int k = 0; k < 5; ++k)
            w[k] = (uint32_t)raw[4 * k] | ((uint32_t)raw[4 * k + 1] << 8) | ((uint32_t)raw[4 * k + 2] << 16) | ((uint32_t)raw[4 * k + 3] << 24);
        chunk_unpack4(w, len, vals);
        for (uint64_t k = 0; k < have; ++k) {
            total += len[k];
            zero = zero || len[k] == 0;
        }
    }
    return chunk_status_of(zero, total, n);
}

// Expands a CHECKED RLE payload into n bytes.
inline void chunk_expand_host(const uint8_t *payload, uint64_t runs, uint8_t *out)
{
    for (uint64_t r = 0; r < runs; ++r) {
        const uint8_t *p = payload + 5 * r;
        const uint32_t len = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        std::memset(out, p[4], len);
        out += len;
    }
}

// Colour + resolve of a decoded chunk at k = 2^lk; output rows of `pitch` pixels.
inline void chunk_resolve_host(const uint32_t *palette, uint32_t lk, const uint8_t *bytes, uint8_t *rgba, uint64_t pitch)
{
    const uint32_t k = 1u << lk, w = kChunkDim >> lk;
    for (uint32_t y = 0; y < w; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            uint32_t s[4] = {0, 0, 0, 0};
            for (uint32_t sy = 0; sy < k; ++sy) {
                const uint8_t *row = bytes + ((size_t)y * k + sy) * kChunkDim + (size_t)x * k;
                for (uint32_t sx = 0; sx < k; ++sx) {
                    const uint32_t c = palette[row[sx]];
                    s[0] += c & 0xffu;
                    s[1] += (c >> 8) & 0xffu;
                    s[2] += (c >> 16) & 0xffu;
                    s[3] += c >> 24;
                }
            }
            const uint32_t c = chunk_mean4(s, lk);
            std::memcpy(rgba + ((size_t)y * pitch + x) * 4u, &c, 4);   // little-endian host, as everywhere in this library
        }
}

// ---- validation and run starts -----------------------------------------------------------------------------------------

// The four records of lane `rec0 / 4`; lengths of records at or beyond `runs` read as 0 (and are not zero runs).
__device__ inline void chunk_load4(const uint32_t *__restrict__ words, uint32_t rec0, uint32_t runs, uint32_t (&len)[4],
                                   uint32_t &vals, bool &zero)
{
    const uint32_t *p = words + (size_t)(rec0 >> 2) * 5u;
    const uint32_t w[5] = {p[0], p[1], p[2], p[3], p[4]};   // inside the scratch: it is padded past the payload
    chunk_unpack4(w, len, vals);
    zero = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool in = rec0 + (uint32_t)k < runs;
        zero = zero || (in && len[k] == 0u);
        len[k] = in ? len[k] : 0u;
    }
}

__global__ __launch_bounds__(kChunkScanThreads) void chunk_block_sums_kernel(const uint32_t *__restrict__ words, uint32_t runs,
                                                                            unsigned long long *__restrict__ block_sum,
                                                                            uint32_t *__restrict__ block_zero)
{
    __shared__ unsigned long long s_sum[kChunkScanThreads / 64];
    __shared__ uint32_t s_zero[kChunkScanThreads / 64];
    const uint32_t rec0 = (blockIdx.x * kChunkScanThreads + threadIdx.x) * 4u;
    unsigned long long sum = 0;
    bool zero = false;
    if (rec0 < runs) {
        uint32_t len[4], vals;
        chunk_load4(words, rec0, runs, len, vals, zero);
        sum = (unsigned long long)len[0] + len[1] + len[2] + len[3];
    }
    sum = wave_sum_u64(sum);
    const unsigned long long zb = __ballot(zero);
    if ((threadIdx.x & 63u) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_zero[threadIdx.x >> 6] = zb != 0ull ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        uint32_t z = 0;
        for (uint32_t w = 0; w < kChunkScanThreads / 64; ++w) {
            t += s_sum[w];
            z |= s_zero[w];
        }
        block_sum[blockIdx.x] = t;
        block_zero[blockIdx.x] = z;
    }
}

// One workgroup: exclusive scan of the block sums in place (64 bits: lengths are arbitrary u32, and a sum that wraps 2^32
// must not pass), and the verdict.  state[0] = the reason code; d_status (may be NULL) receives it too.
__global__ __launch_bounds__(1024) void chunk_scan_sums_kernel(unsigned long long *block_sum, const uint32_t *__restrict__ block_zero,
                                                               uint32_t nblocks, unsigned long long n, uint32_t *state,
                                                               uint32_t *d_status)
{
    __shared__ unsigned long long s_part[1024];
    const uint32_t per = (nblocks + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks, hi = lo + per < nblocks ? lo + per : nblocks;
    unsigned long long sum = 0;
    int zero = 0;
    for (uint32_t k = lo; k < hi; ++k) {
        sum += block_sum[k];
        zero |= (int)block_zero[k];
    }
    s_part[threadIdx.x] = sum;
    const int any_zero = __syncthreads_or(zero);
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 1024; ++t) {
            const unsigned long long v = s_part[t];
            s_part[t] = run;
            run += v;
        }
        const uint32_t st = chunk_status_of(any_zero != 0, run, n);
        state[0] = st;
        if (d_status) *d_status = st;
    }
    __syncthreads();
    unsigned long long run = s_part[threadIdx.x];
    for (uint32_t k = lo; k < hi; ++k) {
        const unsigned long long v = block_sum[k];
        block_sum[k] = run;
        run += v;
    }
}

// starts[r] = min(sum of the lengths before r, n), values[r]: four records per lane, one uint4 + one word per lane.  The clamp
// keeps every start inside [0, n] whatever the stream holds (a valid stream's starts are untouched by it); the 64-bit sums
// cannot wrap (< 2^22 records of < 2^32), so the clamped starts never decrease.
__global__ __launch_bounds__(kChunkScanThreads) void chunk_starts_kernel(const uint32_t *__restrict__ words, uint32_t runs,
                                                                        const unsigned long long *__restrict__ block_off,
                                                                        unsigned long long n, uint32_t *__restrict__ starts,
                                                                        uint32_t *__restrict__ values4)
{
    __shared__ unsigned long long s_wave[kChunkScanThreads / 64];
    const uint32_t rec0 = (blockIdx.x * kChunkScanThreads + threadIdx.x) * 4u;
    uint32_t len[4] = {0, 0, 0, 0}, vals = 0;
    bool zero;
    if (rec0 < runs) chunk_load4(words, rec0, runs, len, vals, zero);
    const unsigned long long mine = (unsigned long long)len[0] + len[1] + len[2] + len[3];
    unsigned long long inc = mine;   // inclusive scan over the wave
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(inc, off, 64);
        if (lane >= (uint32_t)off) inc += up;
    }
    if (lane == 63u) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned long long at = block_off[blockIdx.x] + (inc - mine);
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) at += s_wave[w];
    if (rec0 < runs) {
        uint32_t s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] = (uint32_t)(at < n ? at : n);
            at += len[k];
        }
        *reinterpret_cast<uint4 *>(starts + rec0) = make_uint4(s[0], s[1], s[2], s[3]);   // (the arrays are padded to whole groups)
        values4[rec0 >> 2] = vals;
    }
}

// ---- expansion ---------------------------------------------------------------------------------------------------------

// The last index j in [lo, hi) with a[j] <= x, given a[lo] <= x.
__device__ inline uint32_t chunk_last_le(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t x)
{
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Output-driven: workgroup b owns bytes [b 4096, b 4096 + 4096) of the n output bytes.  Its work does not depend on how the
// bytes are split into runs -- one run of 2^24 and 3.3 M runs of five take the same grid -- and every byte it stores lies in
// its own piece, below n: starts[0] is 0 (an exclusive prefix sum), so the searches always find a run, and the number of
// runs staged is clamped to the LDS arrays (a valid stream never reaches the clamp: its starts are distinct).
__global__ __launch_bounds__(256) void chunk_expand_kernel(const uint32_t *__restrict__ starts, const uint8_t *__restrict__ values,
                                                           uint32_t runs, uint32_t n, uint8_t *__restrict__ out)
{
    __shared__ uint32_t s_start[kChunkPieceRuns + 1];
    __shared__ uint8_t s_val[kChunkPieceRuns + 1];
    const uint32_t p0 = blockIdx.x * kChunkPiece;
    if (p0 >= n) return;
    const uint32_t p1 = n - p0 > kChunkPiece ? p0 + kChunkPiece - 1u : n - 1u;
    const uint32_t j0 = chunk_last_le(starts, 0u, runs, p0);
    // (a valid stream starts at most kChunkPiece - 1 runs behind j0 inside the piece: no need to search further)
    const uint32_t j1 = chunk_last_le(starts, j0, runs - j0 > kChunkPieceRuns + 1u ? j0 + kChunkPieceRuns + 1u : runs, p1);
    const uint32_t cnt = j1 - j0 + 1u < kChunkPieceRuns + 1u ? j1 - j0 + 1u : kChunkPieceRuns + 1u;
    for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
        s_start[i] = starts[j0 + i];
        s_val[i] = values[j0 + i];
    }
    __syncthreads();
    const uint32_t pos = p0 + threadIdx.x * 16u;
    if (pos > p1) return;
    uint32_t i = chunk_last_le(s_start, 0u, cnt, pos);
    uint32_t w[4];
    const uint32_t next = i + 1u < cnt ? s_start[i + 1u] : 0xffffffffu;
    if (next >= pos + 16u) {   // one run covers the lane's 16 bytes
        w[0] = w[1] = w[2] = w[3] = 0x01010101u * s_val[i];
    } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b) {
            while (i + 1u < cnt && s_start[i + 1u] <= pos + b) ++i;
            w[b >> 2] |= (uint32_t)s_val[i] << (8u * (b & 3u));
        }
    }
    uint8_t *dst = out + pos;
    if (pos + 16u <= n && ((uintptr_t)dst & 15u) == 0u) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t b = 0; b < 16u && pos + b < n; ++b) dst[b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
    }
}

// ---- colour + resolve --------------------------------------------------------------------------------------------------

struct ChunkRenderArgs {
    const uint8_t *bytes;      // 4096 x 4096, 256-byte aligned
    const uint32_t *palette;   // 256 words
    uint32_t *out;             // pixel (x, y) at out[y * pitch + x]
    uint64_t pitch;
};

__device__ inline void chunk_stage_palette(uint32_t *s_palette, const uint32_t *palette, uint32_t threads)
{
    for (uint32_t k = threadIdx.x + threadIdx.y * blockDim.x; k < 256u; k += threads) s_palette[k] = palette[k];
    __syncthreads();
}

__device__ inline void chunk_store4(uint32_t *dst, const uint32_t (&px)[4])
{
    if (((uintptr_t)dst & 15u) == 0u) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(px[0], px[1], px[2], px[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = px[k];
    }
}

// k = 2^LK <= 8.  A lane owns four adjacent output pixels: 4 k bytes of each of k rows, one aligned load per row (rows of a
// chunk are 4096 bytes, so every 4 k-byte stretch is naturally aligned); consecutive lanes take consecutive stretches, so a
// wave's loads and its uint4 stores are contiguous.  Sums in RenderSum's packed halves (k^2 x 255 < 2^16 up to k = 8).
template <int LK>
__global__ __launch_bounds__(256) void chunk_resolve_kernel(const ChunkRenderArgs a)
{
    constexpr uint32_t K = 1u << LK, W = kChunkDim >> LK, QUADS = W / 4u, NB = 4u * K;
    __shared__ uint32_t s_palette[256];
    chunk_stage_palette(s_palette, a.palette, 256u);
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;   // the grid is exact: W * QUADS is a multiple of 256
    const uint32_t y = item / QUADS, q = item % QUADS;
    RenderSum sum[4];
#pragma unroll
    for (uint32_t sy = 0; sy < K; ++sy) {
        const uint8_t *row = a.bytes + ((size_t)y * K + sy) * kChunkDim + (size_t)q * NB;
        uint32_t w[NB / 4u];
        if constexpr (NB == 4u) {
            w[0] = *reinterpret_cast<const uint32_t *>(row);
        } else if constexpr (NB == 8u) {
            const uint2 v = *reinterpret_cast<const uint2 *>(row);
            w[0] = v.x;
            w[1] = v.y;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < NB / 16u; ++j) {
                const uint4 v = reinterpret_cast<const uint4 *>(row)[j];
                w[4 * j] = v.x;
                w[4 * j + 1] = v.y;
                w[4 * j + 2] = v.z;
                w[4 * j + 3] = v.w;
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < NB; ++b) sum[b / K].add(s_palette[(w[b >> 2] >> (8u * (b & 3u))) & 0xffu]);
    }
    uint32_t px[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t s[4] = {sum[p].even & 0xffffu, sum[p].odd & 0xffffu, sum[p].even >> 16, sum[p].odd >> 16};
        px[p] = chunk_mean4(s, LK);
    }
    chunk_store4(a.out + (size_t)y * a.pitch + 4u * q, px);
}

// k = 2^LK >= 16.  One lane per pixel would leave 16 waves to read 16 MiB at k = 64, so a pixel is split: a workgroup of
// 256 x 4 lanes owns one output row (k chunk rows); lane (c, part) sums the 16-byte stretch c of the rows sy = part,
// part + 4, ... (a wave's load is 1 KiB of one row, contiguous), at most 16 x 16 x 255 < 2^16 per packed half; the four
// parts meet in LDS as 32-bit sums, and the k / 16 lanes of a pixel in an exchange between neighbouring lanes.
constexpr uint32_t kChunkSplitParts = 4;
template <int LK>
__global__ __launch_bounds__(256 * kChunkSplitParts) void chunk_resolve_split_kernel(const ChunkRenderArgs a)
{
    constexpr uint32_t K = 1u << LK, LANES = K / 16u;   // lanes per pixel: 1, 2, 4
    static_assert(K >= 16u && (K / kChunkSplitParts) * 16u * 255u < 65536u, "the packed halves hold 16 bits");
    __shared__ uint32_t s_palette[256];
    __shared__ uint4 s_part[kChunkSplitParts - 1u][256];
    chunk_stage_palette(s_palette, a.palette, 256u * kChunkSplitParts);
    const uint32_t y = blockIdx.x, c = threadIdx.x, part = threadIdx.y;
    RenderSum sum;
#pragma unroll 4
    for (uint32_t sy = part; sy < K; sy += kChunkSplitParts) {
        const uint4 v = reinterpret_cast<const uint4 *>(a.bytes + ((size_t)y * K + sy) * kChunkDim)[c];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b) sum.add(s_palette[(w[b >> 2] >> (8u * (b & 3u))) & 0xffu]);
    }
    uint32_t s[4] = {sum.even & 0xffffu, sum.odd & 0xffffu, sum.even >> 16, sum.odd >> 16};
    if (part != 0u) s_part[part - 1u][c] = make_uint4(s[0], s[1], s[2], s[3]);
    __syncthreads();
    if (part != 0u) return;
#pragma unroll
    for (uint32_t p = 0; p < kChunkSplitParts - 1u; ++p) {
        const uint4 o = s_part[p][c];
        s[0] += o.x;
        s[1] += o.y;
        s[2] += o.z;
        s[3] += o.w;
    }
#pragma unroll
    for (uint32_t off = 1; off < LANES; off <<= 1) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) s[ch] += __shfl_xor(s[ch], (int)off, 64);
    }
    if (c % LANES == 0u) a.out[(size_t)y * a.pitch + c / LANES] = chunk_mean4(s, LK);
}

// A chunk of one value: w x w pixels of one colour (what chunk_mean4 gives for a uniform block: the colour itself).
__global__ __launch_bounds__(256) void chunk_fill_kernel(uint32_t *out, uint64_t pitch, uint32_t w, uint32_t colour)
{
    const uint32_t quads = w / 4u;   // w is 64 .. 4096
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= w * quads) return;
    const uint32_t px[4] = {colour, colour, colour, colour};
    chunk_store4(out + (size_t)(item / quads) * pitch + 4u * (item % quads), px);
}

inline void launch_chunk_resolve(uint32_t lk, hipStream_t stream, const ChunkRenderArgs &a)
{
    const uint32_t w = kChunkDim >> lk;
    const dim3 flat(w * (w / 4u) / 256u), block(256), rows(w), split(256, kChunkSplitParts);
    switch (lk) {
        case 0: hipLaunchKernelGGL((chunk_resolve_kernel<0>), flat, block, 0, stream, a); break;
        case 1: hipLaunchKernelGGL((chunk_resolve_kernel<1>), flat, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL((chunk_resolve_kernel<2>), flat, block, 0, stream, a); break;
        case 3: hipLaunchKernelGGL((chunk_resolve_kernel<3>), flat, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL((chunk_resolve_split_kernel<4>), rows, split, 0, stream, a); break;
        case 5: hipLaunchKernelGGL((chunk_resolve_split_kernel<5>), rows, split, 0, stream, a); break;
        default: hipLaunchKernelGGL((chunk_resolve_split_kernel<6>), rows, split, 0, stream, a); break;
    }
}

}   // namespace mbk
