// mbk_histogram.h -- histograms of escape counts and the equalisation table built from one (include/mbk.h, "Count histograms
// and histogram-equalised colouring"): hist[c] = the number of samples whose count is c, uint64[mrd], built on the device from
// int32 counts that are already in HBM; and, for the host and for the resolve kernel, the value rule that sends nu through the
// cumulative table.  Nothing here iterates: the counts come from the existing escape kernels.
//
// The histogram kernel is a pure stream of 4 bytes per sample into up to 2^20 bins of 8 bytes (8 MiB: more than LDS holds),
// and the counts of an image are spatially coherent: in an interior block every lane of a wave hits bin 0, around it long runs
// hit the same few bins.  One global atomic per sample would serialise exactly where the data is most common.  What was
// chosen, and why:
//   bin 0      never reaches memory per sample: every lane counts its zeros in a register, a workgroup adds them up in LDS at
//              its end and issues ONE global atomic.  The interior, the largest single bin of most views, costs no atomic.
//   window     a workgroup keeps 32-bit counters for kHistWindow consecutive bins in LDS (48 KiB; two workgroups of 512 lanes
//              per CU leave 64 KiB of the CU's 160 KiB free).  Where the window starts is the workgroup's own choice, made from
//              the smallest non-zero count of its first 2048 samples (a quarter of the window lies below it): a plain view's
//              counts start at 1 and the window is bins 1 .. 12288; a deep view's escaped counts lie in a narrow interval far
//              from 0 (span 1e-60 at mrd 30 000) and the window lands on it.  A wrong guess costs speed only: a count outside
//              the window takes the global path.  Each workgroup reads one contiguous piece of the buffer (a stretch of image
//              rows), so that its first samples say something about the rest.  At its end the workgroup adds its non-zero LDS
//              counters to the table with 64-bit atomics: at most one per bin and workgroup.  A workgroup handles fewer than
//              2^31 samples (the host splits longer buffers), so a 32-bit counter cannot wrap.
//   peeling    before any atomic, LDS or global, a wave takes the value of its first live lane, counts the lanes that hold the
//              same value with one ballot, and the one lane adds the population count; twice per load slot.  A wave whose
//              256 samples are one value issues four atomics (one per slot of its 16-byte loads) instead of 256, and two
//              long runs per slot are folded whatever their values; what is left -- the lanes of a busy boundary, or random
//              data -- issues one atomic per sample, on distinct addresses for the most part.  More rounds cost every wave
//              their ballots and help only runs shorter than a third of a wave.
//   the rest   64-bit global atomics without a return value (global_atomic_add_x2).
//   grid       two workgroups of 512 lanes per CU (four waves per SIMD to hide the loads of a kernel that has nothing else
//              to wait for); fewer when the buffer is short.  More workgroups would multiply the atomics of the final
//              flush (bins in use x workgroups) without adding bandwidth.
// Integer sums have no ordering problem: the table is exact whatever the schedule.  A count outside [0, mrd - 1] is skipped and
// an LDS counter can only be non-zero for a bin below mrd, so nothing is written outside the mrd bins.
//
// Measured on an MI355X against mbk_reduce_counts, the existing kernel that streams the same bytes (scripts/
// histogram_bench.py; profiles/histogram/README.md has the table and the box it ran on), kernel times on 4096^2 / 8192^2
// counts: a buffer of zeros 1.30 / 0.95 x the reduction, of one non-zero value 1.68 / 1.37 x (the case a design with one
// global atomic per sample loses), cfg2's counts 2.49 / 2.08 x (34.9 us for 64 MiB).  Uniformly random counts are 38-43 x at
// mrd 30 000 and 54-63 x at 2^20: nothing folds, most samples miss the window, and the time is that of one 64-bit global
// atomic per sample (about 20 G per second).  No image looks like that; scattered values want another kernel (not built).
//
// Out of scope: fusing the histogram into the escape kernels; histograms of nu itself or of distance values; byte histograms
// of stored chunks (render_level); a sharding form (the table is additive: several GPUs can fill one each and the host adds
// them); slot / submit forms.
#pragma once

#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace mbk {

constexpr uint32_t kHistThreads = 512;
constexpr uint32_t kHistWindow = 12288;        // bins a workgroup keeps in LDS (32-bit counters)
constexpr uint32_t kHistWgPerCu = 2;
constexpr uint64_t kHistLaunchSamples = 1ull << 31;   // per launch: a workgroup's 32-bit counters cannot wrap

struct HistArgs {
    const int32_t *counts;     // n_head scalars, then n4 aligned int4, then n_tail scalars
    uint32_t n_head, n_tail;   // 0 .. 3 each
    uint64_t n4;               // 16-byte groups
    uint64_t per_wg;           // groups per workgroup, a multiple of kHistThreads
    uint32_t mrd;
    unsigned long long *hist;  // mrd bins
};

// One sample that is neither 0 nor out of range, `w` times: the workgroup's LDS window, or the table itself.
__device__ inline void hist_add(uint32_t *s_win, uint32_t base, unsigned long long *hist, uint32_t bin, uint32_t w)
{
    const uint32_t off = bin - base;
    if (off < kHistWindow)
        atomicAdd(&s_win[off], w);
    else
        atomicAdd(&hist[bin], (unsigned long long)w);
}

// One load slot of a wave: x is the lane's count, live whether it takes part (in range, not 0, inside the buffer).
__device__ inline void hist_slot(uint32_t *s_win, uint32_t base, unsigned long long *hist, uint32_t x, bool live, uint32_t lane)
{
    unsigned long long m = __ballot(live);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (m == 0ull) return;
        const uint32_t lead = (uint32_t)__builtin_ctzll(m);
        const uint32_t first = (uint32_t)__shfl((int)x, (int)lead);
        const bool same = live && x == first;
        const unsigned long long mm = __ballot(same);
        if (lane == lead) hist_add(s_win, base, hist, first, (uint32_t)__builtin_popcountll(mm));
        live = live && !same;
        m &= ~mm;
    }
    if (live) hist_add(s_win, base, hist, x, 1u);
}

__global__ __launch_bounds__(kHistThreads) void counts_histogram_kernel(const HistArgs a)
{
    __shared__ uint32_t s_win[kHistWindow];
    __shared__ uint32_t s_min, s_zero;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < kHistWindow; k += kHistThreads) s_win[k] = 0u;
    if (tid == 0) {
        s_min = 0xffffffffu;
        s_zero = 0u;
    }
    __syncthreads();

    const int4 *body = reinterpret_cast<const int4 *>(a.counts + a.n_head);
    const uint64_t g0 = (uint64_t)blockIdx.x * a.per_wg;
    const uint64_t g1 = g0 + a.per_wg < a.n4 ? g0 + a.per_wg : a.n4;   // (g0 <= n4 by the grid's size)
    const uint32_t mrd = a.mrd;
    uint32_t zeros = 0u;

    // the first trip: its smallest live count places the window
    uint64_t g = g0 + tid;
    int4 v = make_int4(0, 0, 0, 0);
    bool have = g < g1;
    if (have) {
        v = body[g];
        uint32_t lo = 0xffffffffu;
        const uint32_t x[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x[k] != 0u && x[k] < mrd && x[k] < lo) lo = x[k];
        if (lo != 0xffffffffu) atomicMin(&s_min, lo);
    }
    __syncthreads();
    const uint32_t lowest = s_min;
    const uint32_t base = (lowest != 0xffffffffu && lowest > kHistWindow / 4u) ? lowest - kHistWindow / 4u : 1u;

    // every wave of the workgroup runs the same number of trips (per_wg is a multiple of the workgroup): no lane leaves
    // before its wave's ballots
    for (uint64_t at = g0; at < g1; at += kHistThreads) {
        int4 next = make_int4(0, 0, 0, 0);
        const uint64_t gn = at + kHistThreads + tid;
        const bool have_next = gn < g1;
        if (have_next) next = body[gn];
        const uint32_t x[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            zeros += (have && x[k] == 0u) ? 1u : 0u;
            hist_slot(s_win, base, a.hist, x[k], have && x[k] != 0u && x[k] < mrd, lane);
        }
        v = next;
        have = have_next;
    }

    // the scalars in front of and behind the aligned body: at most six, straight to the table
    if (blockIdx.x == 0 && tid < a.n_head + a.n_tail) {
        const uint64_t at = tid < a.n_head ? tid : (uint64_t)a.n_head + a.n4 * 4u + (tid - a.n_head);
        const uint32_t x = (uint32_t)a.counts[at];
        if (x < mrd) atomicAdd(&a.hist[x], 1ull);
    }

    if (zeros) atomicAdd(&s_zero, zeros);
    __syncthreads();
    if (tid == 0 && s_zero) atomicAdd(&a.hist[0], (unsigned long long)s_zero);
    for (uint32_t k = tid; k < kHistWindow; k += kHistThreads) {
        const uint32_t c = s_win[k];
        if (c && base + k < mrd) atomicAdd(&a.hist[base + k], (unsigned long long)c);
    }
}

// hist[c] += the number of counts equal to c, for 0 <= c < mrd, on `stream`.  counts: 4-byte aligned; hist: 8-byte aligned
// (the caller checks both).  cus: the device's CU count.
inline void launch_counts_histogram(const int32_t *counts, uint64_t n, uint32_t mrd, unsigned long long *hist, uint32_t cus,
                                    hipStream_t stream)
{
    while (n) {
        const uint64_t part = n < kHistLaunchSamples ? n : kHistLaunchSamples;   // (a multiple of 4: the next part stays aligned)
        HistArgs a;
        a.counts = counts;
        a.n_head = (uint32_t)(((16u - ((uintptr_t)counts & 15u)) & 15u) / 4u);
        if (a.n_head > part) a.n_head = (uint32_t)part;
        a.n4 = (part - a.n_head) / 4u;
        a.n_tail = (uint32_t)((part - a.n_head) % 4u);
        a.mrd = mrd;
        a.hist = hist;
        const uint64_t trips = (a.n4 + kHistThreads - 1u) / kHistThreads;   // of one workgroup, were it alone
        uint64_t grid = (uint64_t)(cus ? cus : 1u) * kHistWgPerCu;
        if (grid > trips) grid = trips ? trips : 1u;
        a.per_wg = (trips + grid - 1u) / grid * kHistThreads;
        grid = a.n4 ? (a.n4 + a.per_wg - 1u) / a.per_wg : 1u;   // (no workgroup starts beyond the body)
        hipLaunchKernelGGL(counts_histogram_kernel, dim3((uint32_t)grid), dim3(kHistThreads), 0, stream, a);
        counts += part;
        n -= part;
    }
}

// The same rule on the host: mbk_counts_histogram_host.
inline void counts_histogram_host(const int32_t *counts, uint64_t n, uint32_t mrd, uint64_t *hist)
{
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t x = (uint32_t)counts[k];
        if (x < mrd) ++hist[x];
    }
}

// The equalisation table (mbk.h): lut[0] = 0, lut[k] = fl((2 cum(k - 1) + h(k - 1)) / (2 E)) for 1 <= k <= mrd + 1.  False if
// 2 E does not stay below 2^53 (the conversions to binary64 would round).  Count 0 takes no part.
inline bool equalize_lut_host(const uint64_t *hist, uint32_t mrd, double *lut)
{
    uint64_t total = 0;
    for (uint32_t c = 1; c < mrd; ++c) {
        if (hist[c] >= (1ull << 52)) return false;
        total += hist[c];
        if (total >= (1ull << 52)) return false;
    }
    lut[0] = 0.0;
    if (total == 0) {
        for (uint32_t k = 1; k <= mrd + 1u; ++k) lut[k] = 0.0;
        return true;
    }
    const double den = (double)(2u * total);
    uint64_t cum = 0;   // cum(k - 1): the counts 1 .. k - 2
    for (uint32_t k = 1; k <= mrd + 1u; ++k) {
        const uint32_t c = k - 1u;
        const uint64_t h = (c >= 1u && c < mrd) ? hist[c] : 0u;
        lut[k] = (double)(2u * cum + h) / den;
        cum += h;
    }
    return true;
}

// The value of one sample under the table (mbk.h, "value"): every operation rounded on its own (the translation unit is
// compiled with -ffp-contract=off).  lut holds mrd + 2 entries; x < mrd + 1 below, so k + 1 <= mrd + 1.
__host__ __device__ inline double equalize_value(const double *lut, uint32_t mrd, double nu)
{
    double x = nu;
    if (!(x >= 0.0)) x = 0.0;   // negative, -inf, NaN
    if (x >= (double)mrd + 1.0) return lut[mrd + 1u];
    const double k = floor(x);
    const double f = x - k;
    const uint32_t i = (uint32_t)k;
    const double d = lut[i + 1u] - lut[i];
    const double p = f * d;
    return lut[i] + p;
}

}   // namespace mbk
