// mbk_api.hip -- host side of libmbk_hip.so: the C ABI declared in include/mbk.h.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see build.py).
// -ffp-contract=off covers the HOST arithmetic in this file too (axis preparation, tile geometry):
// every fp64 operation below must round individually, as CPython / numpy do for the reference
// (DistributedMandelbrotWorkerCUDA.py:24-32,75-78).
#include "../../include/mbk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mbk_kernels.h"
#include "mbk_refill.h"
#include "mbk_persist.h"
#include "mbk_scan.h"
#include "mbk_units.h"
#include "mbk_spill.h"
#include "mbk_feeder.h"
#include "mbk_deep_orbit.h"
#include "mbk_deep.h"
#include "mbk_deep_bla.h"
#include "mbk_deep_wide.h"
#include "mbk_deep_wide_bla.h"
#include "mbk_histogram.h"
#include "mbk_render.h"
#include "mbk_chunks.h"
#include "mbk_distance.h"
#include "mbk_relief.h"
#include "mbk_stripe.h"
#include "mbk_interior.h"
#include "mbk_deep_distance.h"
#include "mbk_deep_distance_bla.h"
#include "mbk_deep_relief.h"
#include "mbk_deep_nucleus.h"
#include "mbk_deep_wide_nucleus.h"
#include "mbk_deep_wide_distance_bla.h"
#include "mbk_deep_wide_relief.h"
#include "mbk_deep_wide_distance.h"
#include "mbk_julia.h"
#include "mbk_julia_distance.h"
#include "mbk_density.h"
#include "mbk_adaptive.h"
#include "mbk_deep_adaptive.h"
#include "mbk_deep_wide_adaptive.h"

using mbk::Axis;
using mbk::ReduceOut;
using mbk::ReduceSlot;
using mbk::TileArgs;
using mbk::WorkQueues;
using mbk::kSafeImagMin;   // (mbk_kernels.h: the literal-doubling threshold, which the refine kernel tests on the device)

// Dispatch lists per stream, used in turn.  Two were enough to let the pre-pass of launch L + 1 run beside the tile kernel of
// launch L -- but a second queue gets no wave slot on a chip full of single-wave workgroups until the tile kernel's grid is
// dealt (measured, profiles/r05/gaps_*.txt: the pre-pass starts 200 us into a 275 us launch and ends after it), which did not
// matter while a launch ended in a 20 us drain and sits on the critical path now that it does not.  With three the pre-pass
// of launch L + 1 may start one launch earlier and is done long before its list is needed.
static const int kOrderRing = 3;

// The dispatch-list ring of one stream: the heavy-first dispatch order of kernels "asm"/"group", kOrderRing lists
// (list | 3 counters | middle-class list) used in turn, so that the pre-pass of a later launch (memset + classify, on the aux
// stream) can run while the tile kernels of the launches before it still read the others
struct OrderRing {
    uint32_t *d_order[kOrderRing] = {};
    uint32_t *d_capture = nullptr;   // the list of every launch captured into a graph on this stream (acquire_order_list), as large as the
                                     // others: written and read on the caller's stream alone, never handed to the pre-pass stream
    uint32_t *d_ctl = nullptr;    // 8 words per list (the ring's, then the capture list's): the units pre-pass' counters (H, V, M | late M,
                                  // settled H, ticket), zero between launches
    bool ctl_dirty = true;        // the counters must be cleared (on the pre-pass' own stream) before the next pre-pass: never used
                                  // yet, or a launch failed after its pre-pass was enqueued and may have left a ticket behind
    size_t order_cap = 0;         // regions
    unsigned order_turn = 0;
    hipStream_t aux = nullptr;    // the pre-pass stream
    uint32_t aux_prio = 0;        // 1 default priority, 2 highest (MBK_OPT_PREPASS_OVERLAP = 2)
    int pp_last = -1;             // MBK_OPT_PREPASS_OVERLAP of the last ordered launch on this stream (a change drains both streams)
    hipEvent_t ev_cls[kOrderRing] = {};   // pre-pass into list k finished
    hipEvent_t ev_done[kOrderRing] = {};  // the tile kernel that read list k finished
    bool done_valid[kOrderRing] = {};

    void drop_lists()   // (the callers of this and the next have drained whatever may still use what goes)
    {
        for (int k = 0; k < kOrderRing; ++k) {
            if (d_order[k]) (void)hipFree(d_order[k]);
            d_order[k] = nullptr;
            done_valid[k] = false;
        }
        if (d_capture) (void)hipFree(d_capture);
        d_capture = nullptr;
        order_cap = 0;
    }
    void drop_aux()   // the stream and the events that tie it to the caller's
    {
        if (aux) (void)hipStreamDestroy(aux);
        aux = nullptr;
        for (int k = 0; k < kOrderRing; ++k) {
            if (ev_cls[k]) (void)hipEventDestroy(ev_cls[k]);
            if (ev_done[k]) (void)hipEventDestroy(ev_done[k]);
            ev_cls[k] = ev_done[k] = nullptr;
            done_valid[k] = false;
        }
    }
    void release()
    {
        if (aux) (void)hipStreamSynchronize(aux);
        drop_lists();
        drop_aux();
        if (d_ctl) (void)hipFree(d_ctl);
        *this = OrderRing();
    }
};

// SPILL (mbk_spill.h): the slots of the spilled lanes (state, meta), the per-block counts, the chunk sums / offsets and the
// total of the prefix sum, the compacted list of slots
struct SpillBuffers {
    void *d_z = nullptr;
    uint32_t *d_meta = nullptr, *d_cnt = nullptr, *d_chunks = nullptr, *d_src = nullptr;
    unsigned long long *d_total = nullptr;
    size_t cap_slots = 0, cap_blocks = 0;   // capacities (slots of 16 bytes of state; blocks)

    void release()
    {
        for (void *q : {d_z, (void *)d_meta, (void *)d_cnt, (void *)d_chunks, (void *)d_src, (void *)d_total})
            if (q) (void)hipFree(q);
        *this = SpillBuffers();
    }
};

// Scratch that helper kernels of a launch use (dispatch-order list, work-queue cursors, the scan
// kernel's deferred-block lists).  It is keyed by the HIP stream the launch goes to: launches on one
// stream are ordered, so one set per stream can never be rewritten while a kernel still reads it,
// however many streams the caller uses (round 1 shared a ring of 8 across all streams).
struct StreamScratch {
    hipStream_t stream = nullptr;
    OrderRing ring;
    WorkQueues *d_queues = nullptr;  // kernel "refill"
    mbk::ScanCursors *d_cursors = nullptr;  // kernel "scan": two sets, used alternately
    uint32_t *d_entries = nullptr;   // kernel "scan": the 64 todo lists (block ids)
    size_t scan_cap_blocks = 0;      // their capacity, in ids
    unsigned scan_turn = 0;
    bool cursors_dirty = false;      // a scan launch failed after its cursor sets were assigned: clear both next time
    uint32_t *h_hint = nullptr;   // pinned, written by the kernels of the last launch on this stream:
                                  // [0] longest deferred list (scan pass 2), [1] share of heavy blocks x 65536
    SpillBuffers spill;
    ReduceSlot *d_red = nullptr;  // mbk_reduce_counts on this (caller) stream: its own partial results, so that a
    ReduceSlot *h_red = nullptr;  // reduction on a caller stream never shares a buffer with a tile in flight on a slot
    // kernel "units": the shares of the eight XCDs (mbk_units.h).  Launch number c (1-based) writes its time stamps into
    // slot c % kStampSlots of h_stamps (pinned) and used the fractions in xcd_ring[c % kShareRing].
    unsigned long long *h_stamps = nullptr;
    double xcd_f[8] = {0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125};
    uint32_t xcd_issued = 0, xcd_consumed = 0;
    struct SharesUsed { uint32_t seq, switches; float f[8]; } xcd_ring[64] = {};   // switches: the ctx' stream_switches at the launch
    // renders (mbk_render.h): the samples of one band, at most MBK_RENDER_BAND_BYTES, and the palette of the last render
    void *d_render = nullptr;
    size_t render_cap = 0;            // bytes
    uint32_t *d_palette = nullptr;    // 65536 entries
    std::vector<uint32_t> palette;    // what d_palette holds
    // stored chunks (mbk_chunks.h): payload | run starts | run values | block sums | block flags | state, sized for chunk_cap_n
    // output bytes; the decoded bytes of the render form; the reason code of the synchronous forms (pinned)
    uint8_t *d_chunk = nullptr;
    size_t chunk_cap_n = 0;
    uint8_t *d_chunk_bytes = nullptr;
    uint32_t *h_chunk_status = nullptr;
    // distance estimates and interior views (mbk_distance.h, mbk_interior.h): the counts of a two-pass launch whose caller wants none
    int32_t *d_dist_counts = nullptr;
    size_t dist_cap_px = 0;
    // equalised renders (mbk_histogram.h): the table of the last one, kept like the palette
    double *d_lut = nullptr;
    size_t lut_cap = 0;               // entries
    std::vector<double> lut;          // what d_lut holds
    // density views (mbk_density.h): the band totals and cursors of the compacted list (64 words), and mbk_density_max's result
    uint32_t *d_density_bands = nullptr;
    mbk::DensityMax *d_density_max = nullptr;
};
static const size_t kMaxStreamScratch = 64;
static const uint32_t kStampSlots = 16, kShareRing = 64;

// One in-flight tile of the host-buffer API: its own stream (so that the D2H of one slot overlaps the
// kernel of the other), events, device result buffers and reduction scratch.
struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr, ev_c0 = nullptr, ev_c1 = nullptr;
    int32_t *d_counts = nullptr;
    uint8_t *d_bytes = nullptr;
    size_t cap_px = 0;
    ReduceSlot *d_red = nullptr;   // mbk::kReduceSlots partial results, folded on the host (reduce_total)
    ReduceSlot *h_red = nullptr;  // pinned copy of d_red
    bool busy = false;           // submitted, not yet waited for
    bool with_bytes = false;
    uint8_t *lazy_h_bytes = nullptr;  // MBK_LAZY_UNIFORM without a copy enqueued at submit: the byte copy is decided in mbk_wait
    size_t lazy_px = 0;
    bool immediate = false;      // MBK_LAZY_UNIFORM, window wholly outside |c| = 2: nothing was enqueued, `imm` is the result
    mbk_stats imm = {};
};

struct mbk_ctx {
    int device = -1;
    Slot s[MBK_SLOTS];
    std::vector<StreamScratch> scratch;  // one per stream seen by this ctx
    size_t last_px = 0;              // pixels of the last tile computed with bytes (for mbk_serialize_last)
    double *d_smooth = nullptr;      // smooth-colouring output of the synchronous API
    size_t smooth_cap_px = 0;
    uint32_t *d_rgba = nullptr;      // the image of the synchronous renders (mbk_*_render_compute)
    size_t rgba_cap_px = 0;
    unsigned long long *d_hist = nullptr;   // the table of the synchronous histograms (mbk_*_histogram_compute)
    size_t hist_cap = 0;             // bins
    uint32_t *d_density = nullptr;   // the table of the synchronous density calls (mbk_view_density_compute, mbk_density_render_compute)
    size_t density_cap = 0;          // cells
    unsigned long long *d_density_stat = nullptr;   // ... and their deposits / dropped points (two words)
    uint8_t *d_rle = nullptr;        // RLE scratch: block counts | run starts | run values | output stream
    size_t rle_cap_px = 0;
    uint32_t opt[MBK_OPT_COUNT_];    // tuning options (mbk_set_option); every value is bit-exact
    hipStream_t last_tile_stream = nullptr;   // launch_tile: the stream of the last tile launch, and how often it changed
    uint32_t stream_switches = 0;             // (xcd_shares_update: which launches had the chip to themselves)
    int scan_occ[2][2] = {{0, 0}, {0, 0}};  // resident single-wave workgroups per CU: [f64|f32][scan|heavy]
    int scan_occ_inline[2] = {0, 0};        // the same for pass 1 in its finish-in-place form (MBK_OPT_SCAN_INLINE)
    uint32_t wave_limit_lds[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // MBK_OPT_WAVE_LIMIT: dynamic LDS bytes per single-wave workgroup
                                            // that leave room for 4 x k workgroups per CU (k = index; 0 = no padding)
    // the host probe of the last window (window_heavy_share): one submit asks for it up to three times -- the copy decision of
    // MBK_LAZY_UNIFORM, the kernel choice, the units rule -- and all three must rest on the same evaluation
    uint32_t spill_launches = 0;              // launches that ran with the SPILL second pass (MBK_INFO_SPILL)
    hipStream_t last_spill_stream = nullptr;  // ... and the stream of the last one
    struct ProbeKey { Axis re, im; uint32_t col0, row0, ncols, nrows; } probe_key = {};
    double probe_share = 0.0;
    bool probe_valid = false;
    // deep-zoom views: this ctx's device copies of the orbits it has used, by orbit id (deep_copy)
    // beside each, the bilinear-approximation tables of the two dcmax it was last launched with (MBK_DEEP_BLA; bla_copy: an
    // adaptive render needs the base view's and the fine view's at once) and the wide table, once a wide view has been
    // launched on the orbit (wide_copy); beside that, the wide bilinear-approximation tables of the two dcmax the MBK_DEEP_XBLA
    // launches last brought (xbla_copy: the same rule, for the same reason)
    struct BlaSlot {
        bool has;
        uint64_t dcmax_bits;
        uint64_t used;                 // bla_clock at the last launch that asked for it: the smaller one is replaced
        double *d_rc;
        double4 *d_ab;
    };
    struct XblaSlot {
        bool has;
        uint64_t dcmax_bits;           // dcmax's mantissa
        int32_t dcmax_exp;             // ... and exponent
        uint64_t used;                 // xbla_clock at the last launch that asked for it: the smaller one is replaced
        int32_t *d_ke;
        mbk::WideBlaEntry *d_ab;
    };
    struct DeepCopy {
        uint64_t id;
        double4 *d;
        mbk::WideEntry *d_wide;
        BlaSlot bla[2];
        uint64_t bla_clock;
        uint32_t levels;               // (the levels and their offsets depend on M alone: the same for every dcmax)
        uint32_t off[mbk::kBlaMaxLevels];
        XblaSlot xbla[2];
        uint64_t xbla_clock;
        uint32_t xlevels;              // (as levels and off: of M alone)
        uint32_t xoff[mbk::kBlaMaxLevels];
    };
    std::vector<DeepCopy> deep;
    bool capturing = false;          // the stream of the launch form being served is capturing a graph (CaptureScope)
    hipDeviceProp_t prop;
    std::string err;
};

struct mbk_deep_orbit {
    mbk::DeepOrbit o;
};

static thread_local std::string g_err;

static int fail(mbk_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    g_err = msg;
    return code;
}

#define MBK_HIP(ctx, call)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            return fail((ctx), MBK_ERR_HIP,                                                 \
                        std::string(#call) + ": " + hipGetErrorString(e_));                 \
        }                                                                                   \
    } while (0)

// ---- graph capture (mbk.h "Graph capture"; DESIGN.md "Graph capture") --------------------------------------------------------

// Is `stream` capturing a graph?  One host call that enqueues nothing.  A status the runtime will not give (the legacy stream
// beside another stream's capture) counts as "no": that call is then no part of any graph.
static bool stream_capturing(hipStream_t stream)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return st != hipStreamCaptureStatusNone;
}

// Every *_launch form opens one of these on the caller's stream before it acquires or enqueues anything: while it lives,
// ctx->capturing tells the steps below -- which do not all see the stream -- that nothing may synchronise, allocate, free or
// copy synchronously, and that everything goes to the caller's stream.  The synchronous and the slot forms open none: their
// streams are the ctx' own and never capture.
struct CaptureScope {
    mbk_ctx *ctx;
    CaptureScope(mbk_ctx *c, hipStream_t stream) : ctx(c) { ctx->capturing = stream_capturing(stream); }
    ~CaptureScope() { ctx->capturing = false; }
    CaptureScope(const CaptureScope &) = delete;
    CaptureScope &operator=(const CaptureScope &) = delete;
};

// The refusal of a call that cannot be served inside a capture.  The places that return it do so before they allocate or
// enqueue anything, so the caller's capture stays valid.
static int refuse_capture(mbk_ctx *ctx, const char *why)
{
    return fail(ctx, MBK_ERR_INVALID, std::string("graph capture: ") + why + " (mbk.h \"Graph capture\")");
}

// Control words inside the stream's scratch (a dispatch list's cursors, the length of the adaptive list, the density band
// counters) put to zero ahead of the kernels that count in them.  Outside a capture a hipMemsetAsync, as ever.  Inside a capture
// a one-workgroup kernel: the second replay of a graph that held the 12-byte memset of a list's cursors ran classify_blocks_kernel
// on the totals the first replay had left -- its light entries, filled in from the back of the list, then leave the list, which
// is a memory fault (tests/test_gpu_graph.py, the ordered "asm" case; profiles/graph_capture/README.md) -- so as far as that
// evidence goes a memset node of a few bytes in the middle of an allocation is not something a replay can rest on, while kernel
// nodes replay in order (the units pre-pass, whose kernel restores its own counters, had passed every replay).
static int clear_words(mbk_ctx *ctx, uint32_t *words, uint32_t n, hipStream_t stream)
{
    if (!ctx->capturing) {
        MBK_HIP(ctx, hipMemsetAsync(words, 0, (size_t)n * sizeof(uint32_t), stream));
        return MBK_OK;
    }
    hipLaunchKernelGGL(mbk::clear_words_kernel, dim3(1), dim3(64), 0, stream, words, n);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- host arithmetic (individually rounded; `volatile` keeps the compiler honest at any -O) ----

static Axis make_axis(double start, double range, uint32_t n)
{
    Axis a;
    std::memset(&a, 0, sizeof(a));
    a.start = start;
    a.n = n;
    volatile double stop = start + range;
    if (n <= 1) {
        a.last = start;
        a.div = 1.0;
        return a;
    }
    volatile double delta = stop - start;
    volatile double div = (double)(n - 1);
    volatile double step = delta / div;
    a.last = stop;
    a.delta = delta;
    a.div = div;
    a.step = step;
    a.step_is_zero = (step == 0.0) ? 1u : 0u;
    return a;
}

static double axis_value_host(const Axis &a, uint32_t k)
{
    if (k + 1u == a.n) return a.last;
    volatile double y;
    if (a.step_is_zero) {
        volatile double q = (double)k / a.div;
        y = q * a.delta;
    } else {
        y = (double)k * a.step;
    }
    volatile double v = y + a.start;
    return v;
}

// Is the pinned last sample of the axis what the regular formula gives anyway, fl(fl((n-1)*step)+start) == stop?
// (np.linspace overwrites y[n-1] with `stop`; for every DataChunk level probed -- and for cfg2's axes -- the
// formula lands on it exactly.)  Then the blocks holding that sample need no special case in the fast paths.
static bool axis_end_is_regular(const Axis &a)
{
    if (a.n <= 1 || a.step_is_zero) return false;
    volatile double y = (double)(a.n - 1u) * a.step;
    volatile double v = y + a.start;
    return v == a.last;
}

// Coordinates must stay far from overflow so that no inf-inf = NaN can appear before the bailout
// test fires (the hand-scheduled kernels compare the high word of |z|^2 as an integer).
static const double kMaxCoord = 0x1p500;

// A multiplier coprime to n near n * (golden ratio - 1): id -> (id * m) mod n is a bijection that
// sends neighbouring ids far apart.
static uint32_t coprime_multiplier(uint32_t n)
{
    if (n < 4) return 1u;
    uint64_t m = (uint64_t)((double)n * 0.6180339887498949);
    if (m < 1) m = 1;
    for (;; ++m) {
        uint64_t a = m, b = n;
        while (b) {
            const uint64_t t = a % b;
            a = b;
            b = t;
        }
        if (a == 1) return (uint32_t)(m % n);
    }
}

// Does a sample k in [k0, k0 + cnt) of the axis have 0 < |value| < 2^-900 (binary32: 2^-100 after the cast)?  Round 1-4
// looked at every sample (4 096 per DataChunk, twice per submitted tile: 10 us of host time where an all-exterior tile costs
// the GPU 25).  The samples before the pinned last one are a monotonic sequence -- k * step is monotonic in k, and so are the
// roundings, the addition of `start` and the cast to float -- so the values nearest to zero sit at the sign change: two
// binary searches find the last sample below zero and the first above it.  (tests: mbk_view_needs_literal_doubling against
// the scan of every sample.)
static bool axis_has_tiny_nonzero(const Axis &a, uint32_t k0, uint32_t cnt, bool f32)
{
    const double thr = f32 ? 0x1p-100 : kSafeImagMin;
    auto value = [&](uint32_t k) { const double y = axis_value_host(a, k); return f32 ? (double)(float)y : y; };
    auto tiny = [&](double y) { return y != 0.0 && std::fabs(y) < thr; };
    if (cnt == 0) return false;
    uint32_t end = k0 + cnt;                    // (k0 + cnt <= a.n: the caller checked the window)
    if (a.n >= 1u && end == a.n) {              // the pinned last sample is not part of the monotonic sequence
        if (tiny(value(a.n - 1u))) return true;
        if (--end == k0) return false;
    }
    const double first = value(k0), last = value(end - 1u);
    if (tiny(first) || tiny(last)) return true;
    if ((first > 0.0 && last > 0.0) || (first < 0.0 && last < 0.0) || first == last) return false;   // no sign change inside
    const double s = last > first ? 1.0 : -1.0;   // s * value(k) is non-decreasing
    auto lower = [&](bool strict) {               // first k in [k0, end) with s * value(k) >= 0 (strict: > 0); end if none
        uint32_t lo = k0, hi = end;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            const double y = s * value(mid);
            if (strict ? y > 0.0 : y >= 0.0) hi = mid;
            else lo = mid + 1u;
        }
        return lo;
    };
    const uint32_t ge = lower(false), gt = lower(true);
    if (ge > k0 && tiny(value(ge - 1u))) return true;     // the last sample on the far side of zero
    if (gt < end && tiny(value(gt))) return true;         // the first one on the near side
    return false;
}

static int validate_view(mbk_ctx *ctx, const mbk_view *v, bool *safe_doubling, bool f32 = false)
{
    if (!v) return fail(ctx, MBK_ERR_INVALID, "view is NULL");
    if (v->width == 0 || v->height == 0) return fail(ctx, MBK_ERR_INVALID, "empty view");
    if (v->ncols == 0 || v->nrows == 0) return fail(ctx, MBK_ERR_INVALID, "empty window");
    if ((uint64_t)v->col0 + v->ncols > v->width || (uint64_t)v->row0 + v->nrows > v->height)
        return fail(ctx, MBK_ERR_INVALID, "window exceeds the view");
    if ((uint64_t)v->ncols * v->nrows > (1ull << 31))
        return fail(ctx, MBK_ERR_INVALID, "window larger than 2^31 pixels");
    const double vals[6] = {v->start_r, v->start_i, v->range_r, v->range_i,
                            v->start_r + v->range_r, v->start_i + v->range_i};
    const double max_coord = f32 ? 0x1p60 : kMaxCoord;
    for (double x : vals)
        if (!std::isfinite(x) || std::fabs(x) > max_coord)
            return fail(ctx, MBK_ERR_INVALID, f32 ? "view coordinates must be finite and |x| <= 2^60 (fp32)"
                                                  : "view coordinates must be finite and |x| <= 2^500");
    *safe_doubling = axis_has_tiny_nonzero(make_axis(v->start_i, v->range_i, v->height), v->row0, v->nrows, f32);
    return MBK_OK;
}

static void free_deep_copy(mbk_ctx::DeepCopy &c)
{
    if (c.d) (void)hipFree(c.d);
    for (mbk_ctx::BlaSlot &b : c.bla) {
        if (b.d_rc) (void)hipFree(b.d_rc);
        if (b.d_ab) (void)hipFree(b.d_ab);
    }
    if (c.d_wide) (void)hipFree(c.d_wide);
    for (mbk_ctx::XblaSlot &b : c.xbla) {
        if (b.d_ke) (void)hipFree(b.d_ke);
        if (b.d_ab) (void)hipFree(b.d_ab);
    }
    c = mbk_ctx::DeepCopy();
}

static void free_scratch(StreamScratch &sc)
{
    sc.ring.release();
    sc.spill.release();
    if (sc.d_queues) (void)hipFree(sc.d_queues);
    if (sc.d_cursors) (void)hipFree(sc.d_cursors);
    if (sc.d_entries) (void)hipFree(sc.d_entries);
    if (sc.h_hint) (void)hipHostFree(sc.h_hint);
    if (sc.h_stamps) (void)hipHostFree(sc.h_stamps);
    if (sc.d_red) (void)hipFree(sc.d_red);
    if (sc.h_red) (void)hipHostFree(sc.h_red);
    if (sc.d_render) (void)hipFree(sc.d_render);
    if (sc.d_palette) (void)hipFree(sc.d_palette);
    if (sc.d_chunk) (void)hipFree(sc.d_chunk);
    if (sc.d_chunk_bytes) (void)hipFree(sc.d_chunk_bytes);
    if (sc.h_chunk_status) (void)hipHostFree(sc.h_chunk_status);
    if (sc.d_dist_counts) (void)hipFree(sc.d_dist_counts);
    if (sc.d_lut) (void)hipFree(sc.d_lut);
    if (sc.d_density_bands) (void)hipFree(sc.d_density_bands);
    if (sc.d_density_max) (void)hipFree(sc.d_density_max);
    sc = StreamScratch();
}

// The scratch set of `stream` (created on first use).  A caller that keeps creating streams would grow
// the table without bound, so past kMaxStreamScratch entries everything is drained and dropped.
static int get_scratch(mbk_ctx *ctx, hipStream_t stream, StreamScratch **out)
{
    for (StreamScratch &sc : ctx->scratch)
        if (sc.stream == stream) {
            *out = &sc;
            return MBK_OK;
        }
    if (ctx->capturing) return refuse_capture(ctx, "the first call of this ctx on a stream allocates its scratch: make the same call once outside the capture");
    if (ctx->scratch.size() >= kMaxStreamScratch) {
        MBK_HIP(ctx, hipDeviceSynchronize());
        for (StreamScratch &sc : ctx->scratch) free_scratch(sc);
        ctx->scratch.clear();
    }
    ctx->scratch.emplace_back();
    StreamScratch &sc = ctx->scratch.back();
    sc.stream = stream;
    *out = &sc;
    MBK_HIP(ctx, hipHostMalloc((void **)&sc.h_hint, 2 * sizeof(uint32_t), hipHostMallocDefault));
    sc.h_hint[0] = sc.h_hint[1] = 0xffffffffu;   // nothing known yet
    return MBK_OK;
}

// Window-dependent launch facts the kernels rely on (computed for the window a launch ACTUALLY covers: the
// edge strips of launch_refill and the bands of a view are windows of their own):
//   fast_bx_end / fast_by_end   leading whole 8x8 blocks that hold no pinned last sample (TileArgs comment);
//   ring_possible               conservative rectangle test against | |c|^2 - 4 | < margin (kernel margins are
//                               1e-9 fp64 / 1e-3 fp32 per pixel; the host test allows 1e-6 / 2e-3);
//   sure_interior               MBK_OPT_SURE_INTERIOR as this launch takes it (sure_interior_word): from the option's value, the
//                               kind of launch (a.mrd, f32, cyc) and the window.  The scan path passes no option: its kernels
//                               do not have the test-free loop.
static void set_window_facts(TileArgs &a, bool f32, bool cyc = true, uint32_t sure_option = 0u);
static void shares_from_fractions(const double *f, uint32_t *cum);
static double window_heavy_share(const TileArgs &a);
static double window_heavy_share(mbk_ctx *ctx, const TileArgs &a);

// Kernel "units": new H fractions for the eight XCDs from the time stamps of the launches on this stream that have finished
// since the last look (mbk_units.h).  A launch that dealt XCD x the fraction f_x of the H list and saw it deal its last
// ids T_x after the launch's first workgroup started measures its speed as f_x / T_x; the fractions follow the normalised
// speeds with a gain of 0.3, clamped to +-12 % of an even deal.  A slot whose 72 stamps do not all carry the launch's
// number (still running, overwritten, a grid too small to reach the tail on the first trip) is skipped -- and so is every
// launch that did not have the chip to itself as far as this ctx can tell: with several streams in flight an XCD's stamps
// say when it found room for this launch among the others, not how fast it is (measured: the fractions then drift the
// wrong way, profiles/r04/xcd_balance_ab.txt), so a launch counts only if no tile launch of the ctx went to another stream
// between the units launch before it and the one after it.
static void xcd_shares_update(const mbk_ctx *ctx, StreamScratch &sc)
{
    const unsigned long long kMask = 0xffffffffffffull;
    uint32_t first = sc.xcd_issued >= kStampSlots ? sc.xcd_issued - kStampSlots + 1u : 1u;
    first = std::max(first, sc.xcd_consumed + 1u);
    for (uint32_t c = first; c <= sc.xcd_issued; ++c) {
        const volatile unsigned long long *st = sc.h_stamps + (size_t)(c % kStampSlots) * mbk::kStampWords;
        const StreamScratch::SharesUsed &used = sc.xcd_ring[c % kShareRing];
        if (used.seq != c) continue;
        const StreamScratch::SharesUsed &before = sc.xcd_ring[(c - 1u) % kShareRing], &after = sc.xcd_ring[(c + 1u) % kShareRing];
        const bool alone = c > 1u && before.seq == c - 1u && before.switches == used.switches &&
                           (c == sc.xcd_issued ? ctx->stream_switches == used.switches : after.seq == c + 1u && after.switches == used.switches);
        unsigned long long v[mbk::kStampWords];
        bool whole = true;
        for (uint32_t i = 0; i < mbk::kStampWords; ++i) {
            v[i] = st[i];
            whole = whole && (v[i] >> 48) == (c & 0xffffu);
        }
        if (!whole) continue;
        unsigned long long start = v[0] & kMask;
        for (uint32_t x = 1; x < 8u; ++x)
            if ((((v[x] & kMask) - start) & kMask) >> 47) start = v[x] & kMask;   // earlier (mod 2^48)
        double T[8], tmin = 1e300, tmax = 0.0, speed[8], sum = 0.0;
        for (uint32_t x = 0; x < 8u; ++x) {
            unsigned long long last = 0;
            for (uint32_t t = 0; t < mbk::kStampTail; ++t)
                last = std::max(last, ((v[8u + x * mbk::kStampTail + t] & kMask) - start) & kMask);
            T[x] = (double)last;
            tmin = std::min(tmin, T[x]);
            tmax = std::max(tmax, T[x]);
        }
        sc.xcd_consumed = c;
        if (!alone || tmin < 1000.0 || tmax > 1.25 * tmin) continue;   // under 10 us, or nothing a share could explain
        for (uint32_t x = 0; x < 8u; ++x) {
            speed[x] = (double)used.f[x] / T[x];
            sum += speed[x];
        }
        double fs = 0.0;
        for (uint32_t x = 0; x < 8u; ++x) {
            const double f = 0.7 * sc.xcd_f[x] + 0.3 * speed[x] / sum;
            sc.xcd_f[x] = std::min(0.14, std::max(0.11, f));
            fs += sc.xcd_f[x];
        }
        for (uint32_t x = 0; x < 8u; ++x) sc.xcd_f[x] /= fs;
    }
}

// The statistics a tile kernel may add up itself: partial-result slots (already zeroed on the launch's stream) to which a
// kernel that can do so adds the tile's pixel-iterations and never-escaped count (the units kernel and the finish-in-place
// light pass).  counts_unwanted: the int32 counts of the launch exist for the statistics only -- a launch that fuses them
// writes none.  fused (out): whether the kernel that served the launch did it.
struct FuseStats { ReduceSlot *slots; bool counts_unwanted; bool fused; };

// The quantised bytes of counts 1..4, packed low byte first: the table of the light paths (units kernel, scan pass 1)
static uint32_t quant_table4(int32_t mrd, bool want_bytes)
{
    uint32_t qtab = 0u;
    if (want_bytes && mrd > 0)
        for (uint32_t c = 1; c <= 4u; ++c)
            qtab |= (uint32_t)(((uint64_t)c * 256u + (uint32_t)mrd - 1u) / (uint32_t)mrd & 0xffu) << (8u * (c - 1u));
    return qtab;
}

// launch_blocks, step by step.  What a launch is made of, decided once from the window and the options:
struct BlockLaunchPlan {
    uint32_t wpw, by;                   // 8x8-pixel blocks (= waves) per workgroup; block rows
    dim3 grid, block;
    uint32_t order_mode, probe_steps;   // MBK_OPT_ORDER, MBK_OPT_PROBE_STEPS
    bool cyc, units, ordered;           // MBK_OPT_CYCLE_DETECT; the units kernel serves the launch; it follows a list built by a pre-pass
    double unit_share;                  // with `units`: the host probe's share of the window still inside after 4 steps
};

// Step 1, the launch facts, the window facts of `a` (set_window_facts) among them.  Host arithmetic only -- no HIP call.
static BlockLaunchPlan block_launch_plan(mbk_ctx *ctx, TileArgs &a, uint32_t kernel, bool safe, bool f32)
{
    BlockLaunchPlan p;
    p.wpw = ctx->opt[MBK_OPT_WAVES_PER_WG];
    a.blocks_x = (a.ncols + 8u * p.wpw - 1u) / (8u * p.wpw);
    p.by = (a.nrows + 7u) / 8u;
    p.cyc = ctx->opt[MBK_OPT_CYCLE_DETECT] != 0u;
    set_window_facts(a, f32, p.cyc, ctx->opt[MBK_OPT_SURE_INTERIOR]);
    p.grid = dim3(a.blocks_x * p.by);
    p.block = dim3(64u * p.wpw);
    p.order_mode = ctx->opt[MBK_OPT_ORDER];
    p.probe_steps = ctx->opt[MBK_OPT_PROBE_STEPS];
    a.perm_mul = p.order_mode == 1 ? coprime_multiplier(p.grid.x) : 1u;
    a.order = nullptr;
    // order 3 = "units" (mbk_units.h): the light blocks of eight neighbouring block columns are ONE workgroup.  Where the
    // units kernel cannot serve a launch (outputs, widths, step counts it has no form for) the launch takes order 2.
    p.units = p.order_mode == 3 && p.wpw == 1u && kernel == MBK_KERNEL_GROUP && !safe && a.smooth == nullptr &&
              (a.counts || a.bytes) && !(a.bytes && a.quant_wide) && a.blocks_x % 8u == 0u && a.blocks_x <= 2048u &&
              a.fast_bx_end > 0u && a.fast_by_end > 0u && (f32 || ctx->opt[MBK_OPT_GROUP_STEPS] == 16u) &&
              p.grid.x >= 16384u && (uint32_t)a.mrd > 2u * p.probe_steps && p.by <= 0xffffu;
    // ... and only where there is light area to batch: the share of the host's 16 x 16 probe pixels of the window that is gone
    // after 4 steps (a deterministic function of the window).  Measured (profiles/r04/units_ab.txt): cfg2 (0.64 light) strict
    // -0.3 % / cycle test +4.7 %, DataChunk (1,0,0) (0.8) +2.1 % / +9.7 %, cfg3 (none) -0.7 % / 0.
    p.unit_share = 0.0;
    if (p.units) {
        p.unit_share = window_heavy_share(ctx, a);
        p.units = (1.0 - p.unit_share) * 65536.0 >= (double)ctx->opt[MBK_OPT_UNITS_MIN_LIGHT];
    }
    // (a list entry packs block row and workgroup column into 16 bits each; wider windows go in image order)
    // heavy-first dispatch order (see classify_blocks_kernel); small launches skip it: one kernel in image
    // order beats memset + classify + tile below ~16 k blocks (cfg1, 4096 blocks: 20 us against 27)
    p.ordered = p.order_mode >= 2 && p.grid.x >= 16384u && (uint32_t)a.mrd > 2u * p.probe_steps && a.blocks_x <= 0xffffu && p.by <= 0xffffu;
    return p;
}

// The dispatch list a launch got from its stream's ring, and the one owner of "the launch took a list and did not get whole":
// leaving launch_blocks before `whole` is set marks the ring's control words for clearing -- a pre-pass that did not run to its
// last workgroup leaves its ticket behind, and no later one would clear it.  (Wider than needed -- a failure before the pre-pass
// is enqueued, or behind the classify pre-pass, marks them too -- which costs the next units launch one drain and one memset.)
struct OrderList {
    StreamScratch *sc = nullptr;   // (null: the launch took no list)
    unsigned k = 0;                // the list's place in the ring
    uint32_t *list = nullptr;      // d_order[k]
    hipStream_t pre = nullptr;     // the stream its pre-pass goes to
    bool overlap = false;          // ... which is the ring's auxiliary stream, tied to the caller's by events
    bool whole = false;
    ~OrderList() { if (sc && !whole) sc->ring.ctl_dirty = true; }
};

// What keeps a captured launch from taking the capture list of `ring`, or NULL.
static const char *capture_list_missing(const OrderRing &ring, uint32_t nblocks, bool units)
{
    if (nblocks > ring.order_cap || !ring.d_capture)
        return "the stream's dispatch lists must grow for this window: make the same call, or a larger one, once outside the capture";
    if (units && (!ring.d_ctl || ring.ctl_dirty))
        return "the units pre-pass' counters must be cleared behind a drain: make the same call once outside the capture";
    return nullptr;
}

static bool capture_list_ready(const mbk_ctx *ctx, hipStream_t stream, uint32_t nblocks, bool units)
{
    for (const StreamScratch &sc : ctx->scratch)
        if (sc.stream == stream) return capture_list_missing(sc.ring, nblocks, units) == nullptr;
    return false;
}

// Step 2, the ring of `stream`: brings it into the state MBK_OPT_PREPASS_OVERLAP asks for (a change drains both streams), grows
// the lists to `nblocks` entries, takes the next one in turn and makes the pre-pass stream wait for that list's last reader.
//
// While `stream` captures a graph (ctx->capturing) none of that happens.  The launch takes the ring's capture list, which no
// launch outside a capture ever takes, and its pre-pass goes to the caller's stream as under MBK_OPT_PREPASS_OVERLAP = 0, whatever
// the option says: the graph is one chain, and a replay writes and reads a list that only work ordered on this stream touches --
// a list of the ring would by then belong to a later launch, whose pre-pass on the auxiliary stream waits for the ring's own
// readers only.  The ring's turn, its mode, its auxiliary stream and its events stay as they are.  A list that would have to
// grow, or (units: the units pre-pass) control words that would have to be allocated or cleared behind a drain, refuse the launch.
static int acquire_order_list(mbk_ctx *ctx, hipStream_t stream, uint32_t nblocks, bool units, OrderList *out)
{
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    OrderRing &ring = sc->ring;
    if (ctx->capturing) {
        if (const char *why = capture_list_missing(ring, nblocks, units)) return refuse_capture(ctx, why);
        out->k = (unsigned)kOrderRing;
        out->list = ring.d_capture;
        out->pre = stream;
        out->overlap = false;
        out->sc = sc;
        return MBK_OK;
    }
    // MBK_OPT_PREPASS_OVERLAP: 0 the pre-pass runs on the caller's stream, in order (one queue, no event: +4..5 us per cfg2
    // launch back to back, profiles/r06/prepass_modes_ab.txt); 1 / 2 on an auxiliary stream (2: at the highest priority), tied
    // to the tile kernel by events.  (Round 6 also tried it as an ANY-ORDER launch on the caller's stream -- an AQL packet
    // without the barrier bit, hipExtAnyOrderLaunch, which would start in the previous tile kernel's drain -- but gfx950
    // ignores the flag: profiles/microbench/anyorder.hip, profiles/r06/anyorder.txt.)
    const uint32_t pp_mode = ctx->opt[MBK_OPT_PREPASS_OVERLAP];
    const bool overlap = pp_mode != 0u;
    // MBK_OPT_PREPASS_OVERLAP = 2: the auxiliary stream has the highest priority, so that the pre-pass of launch L + 1 gets
    // its workgroups in while the tile kernel of launch L is in full swing instead of waiting for its drain (round 5: once
    // the launch no longer ends in a 20 us drain, a pre-pass that waited for it sits on the critical path)
    const uint32_t want_prio = pp_mode == 2u ? 2u : 1u;
    if (ring.pp_last != (int)pp_mode) {
        // the lists' hand-over differs by mode (events between two streams / the order of one queue): nothing of the old
        // mode may be in flight when the first launch of the new one picks its list
        if (ring.pp_last >= 0) {
            MBK_HIP(ctx, hipStreamSynchronize(stream));
            if (ring.aux) MBK_HIP(ctx, hipStreamSynchronize(ring.aux));
        }
        for (int k = 0; k < kOrderRing; ++k) ring.done_valid[k] = false;
        ring.pp_last = (int)pp_mode;
    }
    if (overlap && ring.aux && ring.aux_prio != want_prio) {
        MBK_HIP(ctx, hipStreamSynchronize(stream));
        MBK_HIP(ctx, hipStreamSynchronize(ring.aux));
        ring.drop_aux();
    }
    if (overlap && !ring.aux) {
        if (want_prio == 2u) {
            int least = 0, greatest = 0;
            MBK_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
            MBK_HIP(ctx, hipStreamCreateWithPriority(&ring.aux, hipStreamNonBlocking, greatest));
        } else {
            MBK_HIP(ctx, hipStreamCreateWithFlags(&ring.aux, hipStreamNonBlocking));
        }
        ring.aux_prio = want_prio;
        for (int k = 0; k < kOrderRing; ++k) {
            MBK_HIP(ctx, hipEventCreateWithFlags(&ring.ev_cls[k], hipEventDisableTiming));
            MBK_HIP(ctx, hipEventCreateWithFlags(&ring.ev_done[k], hipEventDisableTiming));
        }
    }
    if (nblocks > ring.order_cap) {
        // the old lists may still be read / written by kernels in flight on the two streams
        MBK_HIP(ctx, hipStreamSynchronize(stream));
        if (ring.aux) MBK_HIP(ctx, hipStreamSynchronize(ring.aux));
        ring.drop_lists();
        // list | 3 counters | middle-class list (classify_blocks_kernel) | 2 counters, the units kernel's plan (64-byte aligned)
        // | its settled H entries (mbk_units.h: units_settled_base)
        for (int k = 0; k < kOrderRing; ++k)
            MBK_HIP(ctx, hipMalloc((void **)&ring.d_order[k], mbk::units_list_words(nblocks) * sizeof(uint32_t)));
        MBK_HIP(ctx, hipMalloc((void **)&ring.d_capture, mbk::units_list_words(nblocks) * sizeof(uint32_t)));
        ring.order_cap = nblocks;
    }
    // Pre-pass of THIS launch on the aux stream: it depends on the window only, not on anything the caller's
    // stream computes, so it may run while the previous launch's tile kernel is still busy (memset + classify
    // are 13 us of a 577 us cfg2 step, with the chip nearly idle).  List k is free once the tile kernel that
    // read it kOrderRing launches ago has finished (ev_done); the tile kernel waits for its list (ev_cls).  With
    // prepass_overlap = 0 everything goes to the caller's stream, as in rounds 1-2.
    const unsigned k = ring.order_turn++ % (unsigned)kOrderRing;
    if (overlap && ring.done_valid[k]) MBK_HIP(ctx, hipStreamWaitEvent(ring.aux, ring.ev_done[k], 0));
    // (serial mode needs no wait: the list's last reader, kOrderRing launches ago, ran on this same stream)
    out->k = k;
    out->list = ring.d_order[k];
    out->pre = overlap ? ring.aux : stream;
    out->overlap = overlap;
    out->sc = sc;   // (from here on `out` marks the ring unless the launch gets whole)
    return MBK_OK;
}

// Step 3a, the pre-pass of the units kernel (mbk_units.h) into list `ol`: clears the ring's control words where they may be
// stale, settles the shares of the eight XCDs and the launch's time-stamp slot (a.plan, a.stamps, a.stamp_tag), enqueues it.
static int enqueue_units_prepass(mbk_ctx *ctx, TileArgs &a, const BlockLaunchPlan &p, const OrderList &ol, hipStream_t stream)
{
    StreamScratch *sc = ol.sc;
    OrderRing &ring = sc->ring;
    // MBK_OPT_M_LATE = s > 0: M blocks whose centre pixel escapes at step >= s open the dispatch order; MBK_OPT_H_SETTLED
    // = k > 0 (with the cycle test only): H blocks whose probe orbit is within 10^-k of settled close the front list
    const uint32_t hs = p.cyc ? ctx->opt[MBK_OPT_H_SETTLED] : 0u;
    const double settle_thr = hs ? std::pow(10.0, -(double)hs) : 0.0;
    // the pre-pass' six counters live apart from the lists (whose layout moves with the window's size), are zeroed once
    // here and put back to zero by the pre-pass itself (mbk_units.h: classify_units_kernel)
    // (inside a capture neither branch is taken: acquire_order_list has refused the launch that would need one)
    if (!ring.d_ctl) {
        MBK_HIP(ctx, hipMalloc((void **)&ring.d_ctl, (size_t)(kOrderRing + 1) * 8u * sizeof(uint32_t)));
        ring.ctl_dirty = true;
    }
    if (ring.ctl_dirty) {
        // ON the stream the pre-pass runs on (a hipMemset on the null stream does not order against a
        // non-blocking stream -- what commit d786d61 removed for the scan cursors), and behind whatever pre-pass may
        // still be running there and on the caller's stream; also after a failed launch (OrderList)
        if (ring.aux) MBK_HIP(ctx, hipStreamSynchronize(ring.aux));
        MBK_HIP(ctx, hipStreamSynchronize(stream));
        MBK_HIP(ctx, hipMemsetAsync(ring.d_ctl, 0, (size_t)(kOrderRing + 1) * 8u * sizeof(uint32_t), ol.pre));
        ring.ctl_dirty = false;
    }
    uint32_t *ctl = ring.d_ctl + 8u * ol.k;
    // the shares of the eight XCDs: MBK_OPT_XCD_BALANCE 0 even, 1 following the stamps of earlier launches on this
    // stream, 2 a fixed uneven deal (tests)
    // (1 applies to the strict loops only: with the cycle test a launch ends with the drain of its boundary blocks, which
    // the stamps -- when an XCD dealt its last ids -- do not see; following them cost 0.3 % there, xcd_balance_ab.txt)
    // (and to a whole chip only: the stamps' "workgroup id mod 8 = XCD" is the dispatch order of 8 XCDs x 32 CUs -- a
    // partitioned device, CPX / DPX modes, deals differently: ADVICE r4)
    // (and never inside a capture: the stamp slot and its tag belong to one enqueue -- a replay would write stale tags into the
    // pinned slots that xcd_shares_update reads -- so a captured launch deals evenly and leaves the shares' bookkeeping alone)
    const uint32_t balance = ctx->opt[MBK_OPT_XCD_BALANCE] == 1u && (p.cyc || ctx->prop.multiProcessorCount != 256 || ctx->capturing)
                                 ? 0u : ctx->opt[MBK_OPT_XCD_BALANCE];
    static const double kUneven[8] = {0.110, 0.140, 0.125, 0.120, 0.130, 0.125, 0.115, 0.135};
    if (balance == 1u && !sc->h_stamps) {
        MBK_HIP(ctx, hipHostMalloc((void **)&sc->h_stamps, (size_t)kStampSlots * mbk::kStampWords * sizeof(unsigned long long),
                                   hipHostMallocDefault));
        std::memset(sc->h_stamps, 0xff, (size_t)kStampSlots * mbk::kStampWords * sizeof(unsigned long long));
    }
    if (balance == 1u) xcd_shares_update(ctx, *sc);
    mbk::XcdShares w;
    double f[8];
    StreamScratch::SharesUsed captured;   // (a captured launch takes no number: it is no launch the stamps could tell of)
    const uint32_t seq = ctx->capturing ? sc->xcd_issued : ++sc->xcd_issued;
    StreamScratch::SharesUsed &used = ctx->capturing ? captured : sc->xcd_ring[seq % kShareRing];
    used.seq = seq;
    used.switches = ctx->stream_switches;
    for (uint32_t x = 0; x < 8u; ++x) {
        f[x] = balance == 1u ? sc->xcd_f[x] : (balance == 2u ? kUneven[x] : 0.125);
        used.f[x] = (float)f[x];
    }
    shares_from_fractions(f, w.cum);
    a.plan = ol.list + ((2u * (size_t)p.grid.x + 5u + 15u) & ~(size_t)15u);   // (ends below units_settled_base: + 16 + 40 <= + 64)
    a.stamps = balance == 1u ? sc->h_stamps + (size_t)(seq % kStampSlots) * mbk::kStampWords : nullptr;
    a.stamp_tag = seq & 0xffffu;
    const uint32_t cwg = ctx->opt[MBK_OPT_CLASSIFY_WG];
    hipLaunchKernelGGL(mbk::classify_units_kernel, dim3((p.grid.x + cwg - 1u) / cwg), dim3(cwg), 0, ol.pre, a, p.grid.x,
                       (int32_t)p.probe_steps, ol.list, ctl, (int32_t)ctx->opt[MBK_OPT_M_LATE], settle_thr, ctl + 3, (uint32_t *)a.plan, w,
                       a.stamps ? 1u : 0u);
    return MBK_OK;
}

// Step 3b, the heavy-first pre-pass (classify_blocks_kernel) into list `ol`, behind the clearing of its cursors.
// *mid_first: the list's middle class is MBK_OPT_M_LATE's and opens the dispatch order.
static int enqueue_classify_prepass(mbk_ctx *ctx, const TileArgs &a, const BlockLaunchPlan &p, const OrderList &ol, bool *mid_first)
{
    const uint32_t nblocks = p.grid.x;
    uint32_t *cursors = ol.list + nblocks;   // right behind the list: the tile kernel finds them at order[gridDim.x]
    const int rc = clear_words(ctx, cursors, 3u, ol.pre);
    if (rc != MBK_OK) return rc;
    // the middle class: MBK_OPT_PROBE_MID's (dispatched between heavy and light) or, without one, MBK_OPT_M_LATE's
    // (order 3 only: boundary blocks whose centre escapes at step >= m_late, dispatched first)
    *mid_first = p.order_mode == 3 && ctx->opt[MBK_OPT_PROBE_MID] > p.probe_steps && ctx->opt[MBK_OPT_M_LATE] >= 2u &&
                 ctx->opt[MBK_OPT_M_LATE] <= p.probe_steps;
    hipLaunchKernelGGL(mbk::classify_blocks_kernel, dim3((nblocks + 1023u) / 1024u), dim3(1024), 0, ol.pre, a,
                       nblocks, 8u * p.wpw, (int32_t)p.probe_steps, (int32_t)(*mid_first ? ctx->opt[MBK_OPT_M_LATE] : ctx->opt[MBK_OPT_PROBE_MID]),
                       ol.list, cursors);
    return MBK_OK;
}

// Step 4a, does the launch run with the SPILL second pass?  SPILL (round 6; mbk_kernels.h: block_pixel_spill, mbk_spill.h): the launches the units kernel does not serve -- deep zooms:
// little light area, long orbits -- with single-wave workgroups, 16-step groups (fp64) and counts / bytes as outputs, when
// the depth and the size are worth a second pass and a checkpoint fits (the per-step prologue + the first checkpoint + 64 steps).
// The second pass lasts at least as long as ONE wave needs for the steps a never-escaping lane has left -- ~ mrd x 21 ns, a
// lone wave issues one dependent instruction per 8 cycles: 0.21 ms at mrd 10 000, 1.05 ms at 50 000 -- whatever the size of the
// launch, while what the first pass saves grows with the number of blocks: the two meet near 2^19 blocks (measured: cfg3,
// 2^20 blocks, +4.7 %; a 16 384 x 1 024 band of cfg4, 2^18 blocks at mrd 50 000, -4 %: profiles/r06/spill_ab.txt), hence
// MBK_OPT_SPILL_MIN_BLOCKS.  Slot numbers are 32 bits, a lane's step count 26.
static bool spill_wanted(const mbk_ctx *ctx, const TileArgs &a, const BlockLaunchPlan &p, uint32_t kernel, bool safe, bool f32)
{
    const uint32_t spill_first = ctx->opt[MBK_OPT_SPILL_FIRST], spill_lanes = ctx->opt[MBK_OPT_SPILL_LANES];
    return !p.units && a.order != nullptr && p.order_mode >= 2u && kernel == MBK_KERNEL_GROUP && !safe && a.smooth == nullptr && p.wpw == 1u &&
           (a.counts || a.bytes) && spill_first != 0u && (f32 || ctx->opt[MBK_OPT_GROUP_STEPS] == 16u) &&
           (uint32_t)a.mrd >= ctx->opt[MBK_OPT_SPILL_MIN_MRD] && (uint32_t)a.mrd < (1u << 26) &&
           ((uint64_t)p.grid.x >> ctx->opt[MBK_OPT_SPILL_MIN_BLOCKS]) != 0ull &&
           (uint64_t)a.mrd > (uint64_t)ctx->opt[MBK_OPT_EXACT_STEPS] + spill_first + 66u &&
           (uint64_t)p.grid.x * spill_lanes < (1ull << 32) && a.fast_bx_end > 0u && a.fast_by_end > 0u;
}

// Step 4b, the SPILL buffers of the stream, grown to `nblocks` blocks, or none (*out).  Where they exist `a` is told about them
// and the blocks' counts are cleared on `stream`.
static int acquire_spill(mbk_ctx *ctx, StreamScratch *sc, hipStream_t stream, TileArgs &a, uint32_t nblocks, SpillBuffers **out)
{
    SpillBuffers &sp = sc->spill;
    const uint32_t spill_lanes = ctx->opt[MBK_OPT_SPILL_LANES];
    const size_t slots = (size_t)nblocks * spill_lanes, nchunks = (nblocks + mbk::kSpillChunk - 1u) / mbk::kSpillChunk;
    *out = nullptr;
    if (slots > sp.cap_slots || nblocks > sp.cap_blocks) {
        MBK_HIP(ctx, hipStreamSynchronize(stream));   // the old buffers may still be in use
        sp.release();
        // 24 bytes per slot (403 MB for an 8192^2 window): a device short of memory runs the launch without the second pass
        // -- an optimisation must not turn into an error -- and the next launch that wants it tries again
        const bool got = hipMalloc(&sp.d_z, slots * 16u) == hipSuccess &&          // (zr, zi) as two doubles; two floats use half of it
                         hipMalloc((void **)&sp.d_meta, slots * sizeof(uint32_t)) == hipSuccess &&
                         hipMalloc((void **)&sp.d_src, slots * sizeof(uint32_t)) == hipSuccess &&
                         hipMalloc((void **)&sp.d_cnt, (size_t)nblocks * sizeof(uint32_t)) == hipSuccess &&
                         hipMalloc((void **)&sp.d_chunks, (nchunks * mbk::kSpillLevels + 1u) * sizeof(uint32_t)) == hipSuccess &&
                         hipMalloc((void **)&sp.d_total, sizeof(unsigned long long)) == hipSuccess;
        if (got) {
            sp.cap_slots = slots;
            sp.cap_blocks = nblocks;
        } else {
            (void)hipGetLastError();   // (the failed allocation's sticky error)
            sp.release();
        }
    }
    if (sp.cap_slots >= slots && sp.cap_blocks >= nblocks && sp.d_z) {
        a.spill_first = ctx->opt[MBK_OPT_SPILL_FIRST];
        a.spill_lanes = spill_lanes;
        a.spill_win_shift = ctx->opt[MBK_OPT_SPILL_CYC_SHIFT];
        a.spill_z = sp.d_z;
        a.spill_meta = sp.d_meta;
        a.spill_cnt = sp.d_cnt;
        MBK_HIP(ctx, hipMemsetAsync(sp.d_cnt, 0, (size_t)nblocks * sizeof(uint32_t), stream));
        *out = &sp;
    }
    return MBK_OK;
}

// Step 5, which instantiation serves a launch: a kernel as a pointer to its launch stub, so that each family has one launch site.
typedef void (*UnitsKernel)(TileArgs, uint32_t);
typedef void (*BlockKernel)(TileArgs);
typedef void (*SpillKernel)(TileArgs, const uint32_t *, const unsigned long long *, uint32_t);

// tile_units_kernel -- rows: number format and cycle test; columns: bytes with the statistics fused | counts and bytes | bytes | counts
static UnitsKernel pick_units_kernel(bool f32, bool cyc, bool stats, bool counts, bool bytes)
{
    static const UnitsKernel forms[4][4] = {
        {mbk::tile_units_kernel<float, 8, true, false, true, true>, mbk::tile_units_kernel<float, 8, true, true, true>,
         mbk::tile_units_kernel<float, 8, true, false, true>, mbk::tile_units_kernel<float, 8, true, true, false>},
        {mbk::tile_units_kernel<float, 8, false, false, true, true>, mbk::tile_units_kernel<float, 8, false, true, true>,
         mbk::tile_units_kernel<float, 8, false, false, true>, mbk::tile_units_kernel<float, 8, false, true, false>},
        {mbk::tile_units_kernel<double, 16, true, false, true, true>, mbk::tile_units_kernel<double, 16, true, true, true>,
         mbk::tile_units_kernel<double, 16, true, false, true>, mbk::tile_units_kernel<double, 16, true, true, false>},
        {mbk::tile_units_kernel<double, 16, false, false, true, true>, mbk::tile_units_kernel<double, 16, false, true, true>,
         mbk::tile_units_kernel<double, 16, false, false, true>, mbk::tile_units_kernel<double, 16, false, true, false>},
    };
    return forms[(f32 ? 0 : 2) + (cyc ? 0 : 1)][stats ? 0 : (counts && bytes) ? 1 : bytes ? 2 : 3];
}

// tile_asm_kernel: the first pass of a SPILL launch, or the form the selector, the literal doubling and MBK_OPT_GROUP_STEPS ask for
static BlockKernel pick_block_kernel(uint32_t kernel, bool safe, bool f32, bool cyc, uint32_t group_steps, bool spill)
{
    if (spill && f32 && cyc) return mbk::tile_asm_kernel<float, true, 8, true, true>;
    if (spill && f32) return mbk::tile_asm_kernel<float, true, 8, false, true>;
    if (spill && cyc) return mbk::tile_asm_kernel<double, true, 16, true, true>;
    if (spill) return mbk::tile_asm_kernel<double, true, 16, false, true>;
    if (f32 && safe) return mbk::tile_asm_kernel<float, false, 0>;
    if (f32 && kernel == MBK_KERNEL_ASM) return mbk::tile_asm_kernel<float, true, 0>;
    if (f32 && cyc) return mbk::tile_asm_kernel<float, true, 8, true>;
    if (f32) return mbk::tile_asm_kernel<float, true, 8>;
    if (safe) return mbk::tile_asm_kernel<double, false, 0>;
    if (kernel == MBK_KERNEL_ASM) return mbk::tile_asm_kernel<double, true, 0>;
    if (group_steps == 32 && !cyc) return mbk::tile_asm_kernel<double, true, 32>;   // (with the cycle test 32 means 16: mbk_loops.inc)
    if (group_steps >= 16 && cyc) return mbk::tile_asm_kernel<double, true, 16, true>;
    if (group_steps >= 16) return mbk::tile_asm_kernel<double, true, 16>;
    if (group_steps == 8 && cyc) return mbk::tile_asm_kernel<double, true, 8, true>;
    if (group_steps == 8) return mbk::tile_asm_kernel<double, true, 8>;
    return mbk::tile_asm_kernel<double, true, 4>;
}

// tile_spill_kernel (mbk_spill.h): the second pass of a SPILL launch
static SpillKernel pick_spill_kernels(bool f32, bool cyc)
{
    if (f32 && cyc) return mbk::tile_spill_kernel<float, true>;
    if (f32) return mbk::tile_spill_kernel<float, false>;
    if (cyc) return mbk::tile_spill_kernel<double, true>;
    return mbk::tile_spill_kernel<double, false>;
}

// ... and the units kernel's launch: its grid, its table of small bytes, and the statistics where the caller takes them from it.
static void enqueue_units_tile(mbk_ctx *ctx, TileArgs &a, const BlockLaunchPlan &p, bool f32, uint32_t lds, hipStream_t stream, FuseStats *fuse)
{
    // Grid: the host cannot know how many units the probe makes of this window, so it estimates them from its own
    // 16 x 16 probe (share of the pixels still inside after 4 steps ~ the H and M blocks; the rest, eight to a unit)
    // and the kernel strides: a deterministic function of the window, no hint from earlier launches.
    const double est = (double)p.grid.x * (p.unit_share + (1.0 - p.unit_share) / 8.0);
    const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
    uint32_t g = (uint32_t)std::min<double>((double)p.grid.x, est * 1.15 + 2048.0);
    // a multiple of 8: id mod 8 = workgroup mod 8 = the XCD; at least 2^14: bounds a wave's trips (the kernel's packed statistics)
    g = (std::max(std::max(g, std::min(p.grid.x, cus * 64u)), 16384u) + 7u) & ~7u;
    a.unit_stride = g;
    const bool stats = fuse != nullptr && fuse->slots != nullptr && fuse->counts_unwanted && a.bytes != nullptr;
    if (stats) {
        a.stats = fuse->slots;
        a.counts = nullptr;
        fuse->fused = true;
    }
    hipLaunchKernelGGL(pick_units_kernel(f32, p.cyc, stats, a.counts != nullptr, a.bytes != nullptr), dim3(g), dim3(64), lds, stream, a,
                       quant_table4(a.mrd, a.bytes != nullptr));
}

// Step 6, the SPILL second pass: compact the blocks' spilled lanes into one list (chunk sums, their scan, the expansion), then run them.
static int enqueue_spill_second_pass(mbk_ctx *ctx, const TileArgs &a, const SpillBuffers &sp, uint32_t nblocks, bool f32, bool cyc, hipStream_t stream)
{
    const uint32_t nchunks = (nblocks + mbk::kSpillChunk - 1u) / mbk::kSpillChunk;
    hipLaunchKernelGGL(mbk::spill_count_kernel, dim3(nchunks), dim3(mbk::kSpillChunk), 0, stream, sp.d_cnt, nblocks, nchunks, sp.d_chunks);
    hipLaunchKernelGGL(mbk::rle_scan_kernel, dim3(1), dim3(1024), 0, stream, sp.d_chunks, nchunks * mbk::kSpillLevels, sp.d_total);
    hipLaunchKernelGGL(mbk::spill_expand_kernel, dim3(nchunks), dim3(mbk::kSpillChunk), 0, stream, sp.d_cnt, nblocks, nchunks,
                       sp.d_chunks, a.spill_lanes, sp.d_src);
    // grid: an upper bound (the number of lanes is known on the device only), strided
    const uint32_t nwg = (uint32_t)std::min<uint64_t>(((uint64_t)nblocks * a.spill_lanes + 63u) / 64u, 16384u);
    // (fewer resident waves per SIMD for this pass -- through unused LDS, as MBK_OPT_WAVE_LIMIT -- were tried: 2 / 3 per SIMD cost
    // 0.1 / 0.05 ms of its 0.64 ms; what halved it was the order of the list, latest checkpoint first: profiles/r06/spill_ab.txt)
    const uint32_t lds2 = 0u;
    hipLaunchKernelGGL(pick_spill_kernels(f32, cyc), dim3(nwg), dim3(64), lds2, stream, a, sp.d_src, sp.d_total, nwg);
    MBK_HIP(ctx, hipGetLastError());
    ++ctx->spill_launches;
    ctx->last_spill_stream = stream;
    return MBK_OK;
}

// Launch the one-wave-per-block kernels ("asm" / "group", fp64 or fp32) for the window described by `a`
// (a.col0/row0/ncols/nrows, output at a.out_*), optionally behind the heavy-first classify pre-pass: the steps above, in order.
// list_optional (inside a capture only; launch_tile: the default selector in place of the two-pass "scan"): where the capture
// list is not there for the taking the launch goes in image order instead of being refused.
static int launch_blocks(mbk_ctx *ctx, TileArgs a, uint32_t kernel, bool safe, bool f32, hipStream_t stream, FuseStats *fuse = nullptr,
                         bool list_optional = false)
{
    BlockLaunchPlan p = block_launch_plan(ctx, a, kernel, safe, f32);
    if (p.ordered && list_optional && ctx->capturing && !capture_list_ready(ctx, stream, p.grid.x, p.units)) p.ordered = p.units = false;
    OrderList ol;   // (once it holds a list, a failing return leaves the ring marked: ctl_dirty)
    if (p.ordered) {
        int rc = acquire_order_list(ctx, stream, p.grid.x, p.units, &ol);
        if (rc != MBK_OK) return rc;
        OrderRing &ring = ol.sc->ring;
        bool mid_first = false;
        rc = p.units ? enqueue_units_prepass(ctx, a, p, ol, stream) : enqueue_classify_prepass(ctx, a, p, ol, &mid_first);
        if (rc != MBK_OK) return rc;
        if (ol.overlap) {
            MBK_HIP(ctx, hipEventRecord(ring.ev_cls[ol.k], ring.aux));
            MBK_HIP(ctx, hipStreamWaitEvent(stream, ring.ev_cls[ol.k], 0));
        }
        a.order = ol.list;
        a.ngrid = p.grid.x;
        a.order_mid = mid_first ? 2u : (ctx->opt[MBK_OPT_PROBE_MID] <= p.probe_steps ? 1u : 0u);
    }
    SpillBuffers *spill = nullptr;
    // (not inside a capture: the buffers may have to grow behind a drain, and every kernel stores the same results)
    if (!ctx->capturing && spill_wanted(ctx, a, p, kernel, safe, f32)) {
        const int rc = acquire_spill(ctx, ol.sc, stream, a, p.grid.x, &spill);
        if (rc != MBK_OK) return rc;
    }
    // MBK_OPT_WAVE_LIMIT: unused dynamic LDS caps the resident waves per SIMD (single-wave workgroups only)
    const uint32_t lds = p.wpw == 1u ? ctx->wave_limit_lds[ctx->opt[MBK_OPT_WAVE_LIMIT] & 7u] : 0u;
    if (p.units && a.order)
        enqueue_units_tile(ctx, a, p, f32, lds, stream, fuse);
    else
        hipLaunchKernelGGL(pick_block_kernel(kernel, safe, f32, p.cyc, ctx->opt[MBK_OPT_GROUP_STEPS], spill != nullptr), p.grid, p.block, lds, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, MBK_ERR_HIP, std::string("tile launch: ") + hipGetErrorString(e));
    if (ol.overlap) {   // list `ol.k` is busy until this tile kernel has finished
        MBK_HIP(ctx, hipEventRecord(ol.sc->ring.ev_done[ol.k], stream));
        ol.sc->ring.done_valid[ol.k] = true;
    }
    if (spill) {
        const int rc = enqueue_spill_second_pass(ctx, a, *spill, p.grid.x, f32, p.cyc, stream);
        if (rc != MBK_OK) return rc;
    }
    ol.whole = true;
    return MBK_OK;
}

// Can any pixel of the window lie within the ring | |c|^2 - 4 | < 1e-6 ?  (conservative rectangle test)
static bool window_may_touch_ring(const TileArgs &a, double margin = 1e-6)
{
    const double x0 = axis_value_host(a.re, a.col0), x1 = axis_value_host(a.re, a.col0 + a.ncols - 1u);
    const double y0 = axis_value_host(a.im, a.row0), y1 = axis_value_host(a.im, a.row0 + a.nrows - 1u);
    const double xlo = std::fmin(x0, x1), xhi = std::fmax(x0, x1), ylo = std::fmin(y0, y1), yhi = std::fmax(y0, y1);
    const double dx = (xlo <= 0.0 && 0.0 <= xhi) ? 0.0 : std::fmin(std::fabs(xlo), std::fabs(xhi));
    const double dy = (ylo <= 0.0 && 0.0 <= yhi) ? 0.0 : std::fmin(std::fabs(ylo), std::fabs(yhi));
    const double fx = std::fmax(std::fabs(xlo), std::fabs(xhi)), fy = std::fmax(std::fabs(ylo), std::fabs(yhi));
    const double rmin2 = dx * dx + dy * dy, rmax2 = fx * fx + fy * fy;
    return !(rmax2 < 4.0 - margin || rmin2 > 4.0 + margin);
}

// MBK_OPT_SURE_INTERIOR as one launch takes it (TileArgs::sure_interior): non-zero only for a strict fp64 launch of at least 64
// steps whose window can hold certified blocks at all -- its rectangle meets the box [-1.3, 0.4] x [-0.7, 0.7] around the main
// cardioid and the period-2 disk, and one of the 16 x 16 probe pixels of window_heavy_share's grid passes the certificate.  A deep
// zoom beside the set lies inside that box and holds no such pixel; it, like an all-exterior tile, must not pay 14 instructions
// per heavy block for a certificate that never holds.  A window whose certified area falls between the probe pixels (under
// 1/256 of it) merely keeps today's path.  Force mode (2) ignores the window.  A deterministic function of its arguments.
static uint32_t sure_interior_word(const TileArgs &a, bool f32, bool cyc, uint32_t option)
{
    if (option == 0u || f32 || cyc || a.mrd < 65) return 0u;
    if (option == 2u) return 2u;
    if (a.ncols == 0u || a.nrows == 0u) return 0u;
    const double x0 = axis_value_host(a.re, a.col0), x1 = axis_value_host(a.re, a.col0 + a.ncols - 1u);
    const double y0 = axis_value_host(a.im, a.row0), y1 = axis_value_host(a.im, a.row0 + a.nrows - 1u);
    const double xlo = std::fmin(x0, x1), xhi = std::fmax(x0, x1), ylo = std::fmin(y0, y1), yhi = std::fmax(y0, y1);
    if (!(xlo <= 0.4 && xhi >= -1.3 && ylo <= 0.7 && yhi >= -0.7)) return 0u;
    const uint32_t k = 16;
    for (uint32_t j = 0; j < k; ++j) {
        const double ci = axis_value_host(a.im, a.row0 + (uint32_t)(((uint64_t)(2u * j + 1u) * a.nrows) / (2u * k)));
        for (uint32_t i = 0; i < k; ++i)
            if (mbk::sure_interior_point(axis_value_host(a.re, a.col0 + (uint32_t)(((uint64_t)(2u * i + 1u) * a.ncols) / (2u * k))), ci))
                return 1u;
    }
    return 0u;
}

static void set_window_facts(TileArgs &a, bool f32, bool cyc, uint32_t sure_option)
{
    a.sure_interior = sure_interior_word(a, f32, cyc, sure_option);
    a.ring_possible = window_may_touch_ring(a, f32 ? 2e-3 : 1e-6) ? 1u : 0u;
    a.fast_bx_end = a.fast_by_end = 0u;
    if (a.re.step_is_zero || a.im.step_is_zero) return;
    // window columns / rows before the axis' last sample (col0 + ncols <= n: validate_view); the last sample itself
    // counts when the regular formula reproduces it (axis_end_is_regular)
    const uint64_t re_n = (uint64_t)a.re.n - (axis_end_is_regular(a.re) ? 0u : 1u), im_n = (uint64_t)a.im.n - (axis_end_is_regular(a.im) ? 0u : 1u);
    const uint64_t cols_ok = std::min<uint64_t>(a.ncols, re_n - std::min<uint64_t>(a.col0, re_n));
    const uint64_t rows_ok = std::min<uint64_t>(a.nrows, im_n - std::min<uint64_t>(a.row0, im_n));
    a.fast_bx_end = (uint32_t)(cols_ok / 8u);
    a.fast_by_end = (uint32_t)(rows_ok / 8u);
}

// Kernel "refill": persistent lane-refill kernel on the interior blocks + "group" on the edge strips.
// Falls back to "group" for everything the narrow persistent kernel excludes (see mbk_persist.h).
static int launch_refill(mbk_ctx *ctx, const TileArgs &a, bool safe, hipStream_t stream)
{
    if (ctx->capturing) return refuse_capture(ctx, "MBK_KERNEL_REFILL is not served inside a capture: take the default selector, group or asm");
    const bool eligible = !safe && a.mrd >= 2 && a.counts != nullptr && !a.re.step_is_zero &&
                          !a.im.step_is_zero && !window_may_touch_ring(a, 1e-6);
    // interior = whole 8x8 blocks that do not contain the last sample of either axis
    const uint32_t cols_ok = a.re.n > 0 ? std::min<uint64_t>(a.ncols, (uint64_t)(a.re.n - 1u) - std::min<uint64_t>(a.col0, a.re.n - 1u)) : 0u;
    const uint32_t rows_ok = a.im.n > 0 ? std::min<uint64_t>(a.nrows, (uint64_t)(a.im.n - 1u) - std::min<uint64_t>(a.row0, a.im.n - 1u)) : 0u;
    const uint32_t icols = eligible ? (cols_ok / 8u) * 8u : 0u, irows = eligible ? (rows_ok / 8u) * 8u : 0u;
    if (icols == 0 || irows == 0) return launch_blocks(ctx, a, MBK_KERNEL_GROUP, safe, false, stream);

    mbk::PersistArgs q;
    std::memset(&q, 0, sizeof(q));
    q.re_start = a.re.start;
    q.re_step = a.re.step;
    q.im_start = a.im.start;
    q.im_step = a.im.step;
    q.col0 = a.col0;
    q.row0 = a.row0;
    q.pitch = a.out_pitch;
    q.bxn = icols / 8u;
    q.nblocks = q.bxn * (irows / 8u);
    q.total = (uint32_t)a.mrd - 1u;
    q.livemin = ctx->opt[MBK_OPT_RF_LIVEMIN];
    q.patience = ctx->opt[MBK_OPT_RF_PATIENCE];
    q.batch = ctx->opt[MBK_OPT_RF_BATCH];
    q.counts = a.counts;
    StreamScratch *sc = nullptr;
    int rcs = get_scratch(ctx, stream, &sc);
    if (rcs != MBK_OK) return rcs;
    if (!sc->d_queues) MBK_HIP(ctx, hipMalloc((void **)&sc->d_queues, sizeof(WorkQueues)));
    WorkQueues *wq = sc->d_queues;
    hipLaunchKernelGGL(mbk::init_queues_kernel, dim3(1), dim3(64), 0, stream, wq, q.nblocks);
    uint32_t waves = (uint32_t)ctx->prop.multiProcessorCount * 4u * ctx->opt[MBK_OPT_RF_WAVES];
    if (waves > q.nblocks) waves = q.nblocks;
    hipLaunchKernelGGL(mbk::tile_persist_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, stream, q, wq);
    MBK_HIP(ctx, hipGetLastError());
    // edge strips through the ordinary kernel, written into the same output image
    TileArgs e = a;
    e.bytes = nullptr;
    if (icols < a.ncols) {  // right strip, all rows
        e.col0 = a.col0 + icols;
        e.ncols = a.ncols - icols;
        e.out_col0 = a.out_col0 + icols;
        int rc = launch_blocks(ctx, e, MBK_KERNEL_GROUP, safe, false, stream);
        if (rc != MBK_OK) return rc;
    }
    if (irows < a.nrows) {  // bottom strip, interior columns only
        e = a;
        e.bytes = nullptr;
        e.ncols = icols;
        e.row0 = a.row0 + irows;
        e.nrows = a.nrows - irows;
        e.out_row0 = a.out_row0 + irows;
        int rc = launch_blocks(ctx, e, MBK_KERNEL_GROUP, safe, false, stream);
        if (rc != MBK_OK) return rc;
    }
    if (a.bytes) {
        const uint64_t npx = (uint64_t)a.ncols * a.nrows;
        hipLaunchKernelGGL(mbk::quantise_kernel, dim3(2048), dim3(256), 0, stream, a.counts, a.bytes, npx, a.mrd,
                           a.quant_wide, a.quant_rcp);
        MBK_HIP(ctx, hipGetLastError());
    }
    return MBK_OK;
}

// Share of the window that the light pass of kernel "scan" would NOT finish: a 16 x 16 grid of its pixels is
// iterated on the host for the 4 steps pass 1 runs (~1 000 steps, a few microseconds -- a launch costs more), and the
// fraction still inside is returned.  A scheduling heuristic only (kernel choice of MBK_KERNEL_DEFAULT): plain
// host doubles, no claim of bit-exactness, results never depend on it.
static double window_heavy_share(const TileArgs &a)
{
    const uint32_t k = 16;
    uint32_t inside = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const double ci = axis_value_host(a.im, a.row0 + (uint32_t)(((uint64_t)(2u * j + 1u) * a.nrows) / (2u * k)));
        for (uint32_t i = 0; i < k; ++i) {
            const double cr = axis_value_host(a.re, a.col0 + (uint32_t)(((uint64_t)(2u * i + 1u) * a.ncols) / (2u * k)));
            double zr = cr, zi = ci;
            bool in = true;
            for (int n = 0; n < 4 && in; ++n) {
                const double t = zr * zr - zi * zi + cr;
                zi = 2.0 * zr * zi + ci;
                zr = t;
                in = zr * zr + zi * zi < 4.0;
            }
            inside += in ? 1u : 0u;
        }
    }
    return (double)inside / (double)(k * k);
}

// ... evaluated once per window: the last window's answer is kept on the ctx
static double window_heavy_share(mbk_ctx *ctx, const TileArgs &a)
{
    mbk_ctx::ProbeKey k;
    std::memset(&k, 0, sizeof(k));
    k.re = a.re;
    k.im = a.im;
    k.col0 = a.col0;
    k.row0 = a.row0;
    k.ncols = a.ncols;
    k.nrows = a.nrows;
    if (ctx->probe_valid && std::memcmp(&k, &ctx->probe_key, sizeof(k)) == 0) return ctx->probe_share;
    ctx->probe_key = k;
    ctx->probe_share = window_heavy_share(a);
    ctx->probe_valid = true;
    return ctx->probe_share;
}

// The kernels of "scan" (mbk_scan.h), as for launch_blocks.  tile_light_kernel -- rows: finish in place with the statistics fused,
// cycle test / strict | finish in place, cycle test / strict | listing what it cannot finish; columns: counts and bytes | bytes | counts
typedef void (*ScanKernel)(TileArgs, mbk::ScanArgs);
template <typename T>
static ScanKernel pick_light_kernel(int inl, bool stats, bool counts, bool bytes)
{
    static const ScanKernel forms[5][3] = {
        {mbk::tile_light_kernel<T, true, true, 2, true>, mbk::tile_light_kernel<T, false, true, 2, true>, mbk::tile_light_kernel<T, true, false, 2, true>},
        {mbk::tile_light_kernel<T, true, true, 1, true>, mbk::tile_light_kernel<T, false, true, 1, true>, mbk::tile_light_kernel<T, true, false, 1, true>},
        {mbk::tile_light_kernel<T, true, true, 2>, mbk::tile_light_kernel<T, false, true, 2>, mbk::tile_light_kernel<T, true, false, 2>},
        {mbk::tile_light_kernel<T, true, true, 1>, mbk::tile_light_kernel<T, false, true, 1>, mbk::tile_light_kernel<T, true, false, 1>},
        {mbk::tile_light_kernel<T, true, true, 0>, mbk::tile_light_kernel<T, false, true, 0>, mbk::tile_light_kernel<T, true, false, 0>},
    };
    return forms[inl == 0 ? 4 : (stats ? 0 : 2) + (inl == 2 ? 0 : 1)][(counts && bytes) ? 0 : bytes ? 1 : 2];
}

template <typename T>
static ScanKernel pick_todo_kernel(bool cyc) { return cyc ? mbk::tile_todo_kernel<T, true> : mbk::tile_todo_kernel<T, false>; }

// The two-pass form's scratch on `stream`: the cursor set of this launch and the one its pass 1 clears for the next, the 64
// todo lists (`qcap` ids each) and the size of pass 2, into `s`.
static int acquire_scan_lists(mbk_ctx *ctx, hipStream_t stream, uint32_t qcap, double probe_share, mbk::ScanArgs &s, StreamScratch **out)
{
    // (launch_tile sends no captured launch here: the sets alternate per enqueue, and the hint below is read at enqueue time)
    if (ctx->capturing) return refuse_capture(ctx, "the two-pass form of MBK_KERNEL_SCAN is not served inside a capture");
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    if (!sc->d_cursors || sc->cursors_dirty) {
        if (!sc->d_cursors) MBK_HIP(ctx, hipMalloc((void **)&sc->d_cursors, 2 * sizeof(mbk::ScanCursors)));
        // once per stream, ON that stream: hipMemset on the null stream does not order against a
        // non-blocking stream (the first launch on a new stream raced with it and lost listed blocks).
        // Also after a failed launch: pass 1 of launch L is what clears the set of launch L+1, so a launch that
        // failed after taking its sets would leave the next one appending behind stale tails.
        MBK_HIP(ctx, hipMemsetAsync(sc->d_cursors, 0, 2 * sizeof(mbk::ScanCursors), stream));
        sc->scan_turn = 0;
        sc->cursors_dirty = false;
    }
    const size_t need = (size_t)qcap * mbk::kScanQueues;
    if (need > sc->scan_cap_blocks) {
        if (sc->d_entries) {
            MBK_HIP(ctx, hipStreamSynchronize(stream));  // may still be in use
            (void)hipFree(sc->d_entries);
        }
        sc->d_entries = nullptr;
        sc->scan_cap_blocks = 0;
        MBK_HIP(ctx, hipMalloc((void **)&sc->d_entries, need * sizeof(uint32_t)));
        sc->scan_cap_blocks = need;
    }
    s.cur = sc->d_cursors + (sc->scan_turn & 1u);
    s.cur_next = sc->d_cursors + ((sc->scan_turn + 1u) & 1u);
    ++sc->scan_turn;
    s.entries = sc->d_entries;
    s.qcap = qcap;
    // pass 2: 64 lists x (hint = longest list of the previous launch on this stream + 25 %).  Never fewer
    // workgroups than fill the chip (when the tile has that many blocks): a hint from a light tile followed by
    // a heavy one would otherwise leave a few waves looping over whole lists.
    // When the host probe of THIS window (window_heavy_share) found no pixel that outlives the light pass and the
    // finish-in-place form is switched off, pass 2 is launched as one workgroup per CU (its stride loop keeps it correct
    // if the probe missed a thin feature) instead of the chip-filling floor.
    const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
    const uint32_t hint = sc->h_hint[0];
    if (probe_share == 0.0) {
        s.ranks2 = std::min(qcap, (cus + mbk::kScanQueues - 1u) / mbk::kScanQueues);
    } else {
        s.ranks2 = hint == 0xffffffffu ? qcap : (uint32_t)std::min<uint64_t>(qcap, (uint64_t)hint + hint / 4u + 2u);
        s.ranks2 = std::max(s.ranks2, std::min(qcap, (cus * 32u + mbk::kScanQueues - 1u) / mbk::kScanQueues));
    }
    if (s.ranks2 == 0u) s.ranks2 = 1u;
    s.hint_out = sc->h_hint;
    *out = sc;
    return MBK_OK;
}

// Kernel "scan": a persistent light pass over every 8x8 block, then one workgroup per block it listed as
// unfinished (mbk_scan.h).  Launches the light pass cannot serve go to launch_blocks ("group").
template <typename T>
static int launch_scan_t(mbk_ctx *ctx, TileArgs a, bool safe, hipStream_t stream, double probe_share, FuseStats *fuse = nullptr)
{
    const bool f32 = sizeof(T) == 4;
    const bool cyc = ctx->opt[MBK_OPT_CYCLE_DETECT] != 0u;
    a.blocks_x = (a.ncols + 7u) / 8u;
    const uint32_t nby = (a.nrows + 7u) / 8u;
    const uint32_t nblocks = a.blocks_x * nby;  // <= 2^31 / 64 (validate_view)
    const uint32_t total_steps = a.mrd > 1 ? (uint32_t)a.mrd - 1u : 0u;
    // Pass 1 is a persistent grid: exactly as many single-wave workgroups as are resident at once (a second
    // round of a statically strided pass would double its time) -- what the occupancy query reports for the
    // kernel, capped by the scan_waves option -- rounded down to whole block rows.
    const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
    // Nothing of the window's probe grid outlives the light pass (probe_share == 0: an all-exterior tile): pass 1
    // finishes its own leftovers and there is no pass 2 (tile_light_kernel, kInline)
    const bool inline_todo = probe_share == 0.0 && ctx->opt[MBK_OPT_SCAN_INLINE] != 0u;
    const uint32_t per_cu = std::min<uint32_t>(4u * ctx->opt[MBK_OPT_SCAN_WAVES],
                                               (uint32_t)(inline_todo ? ctx->scan_occ_inline[f32 ? 1 : 0] : ctx->scan_occ[f32 ? 1 : 0][0]));
    const uint32_t wmax = cus * per_cu;
    if (safe || a.re.step_is_zero || a.im.step_is_zero || a.smooth != nullptr || (a.bytes && a.quant_wide) ||
        total_steps < 4u || !(a.counts || a.bytes) || a.blocks_x > wmax)
        return launch_blocks(ctx, a, MBK_KERNEL_GROUP, safe, f32, stream);

    mbk::ScanArgs s;
    std::memset(&s, 0, sizeof(s));
    // Row strips (mbk_scan.h): in the finish-in-place form a wave's region is 64 x 1 pixels instead of an 8x8 block, so that
    // every store instruction writes one contiguous piece of a row; the fields below then count strips and rows.  Not for
    // narrow windows (the ragged last strip of a row runs with idle lanes).
    const bool strip = inline_todo && ctx->opt[MBK_OPT_SCAN_STRIP] != 0u && a.ncols >= 512u;
    const uint32_t regions_x = strip ? (a.ncols + 63u) / 64u : a.blocks_x, regions_y = strip ? a.nrows : nby, region_h = strip ? 1u : 8u;
    s.strip = strip ? 1u : 0u;
    s.strips_x = regions_x;
    s.stride_by = std::min(wmax / regions_x, regions_y);
    // (pass 1 addresses a run of blocks through a 32-bit lane offset that advances by this much per block)
    if ((uint64_t)s.stride_by * region_h * a.out_pitch * 4u >= (1ull << 31)) return launch_blocks(ctx, a, MBK_KERNEL_GROUP, safe, f32, stream);
    const uint32_t w1 = s.stride_by * regions_x;
    s.nblocks = nblocks;
    // XCD-aware column order (profiles/microbench/light_path.hip: the 8x8 store pattern of a 4096^2 int32 tile
    // takes 25.6 us in image order -- each 128-byte line is written by four XCDs -- and 12.9 us with it)
    s.xcd_map = (!strip && ctx->opt[MBK_OPT_SCAN_XCD_MAP] != 0u && a.blocks_x % 32u == 0u) ? 1u : 0u;
    // column jump: ~5/16 of the width, a multiple of 32 columns when the XCD map is on (keeps its grouping).  It
    // spreads the unfinished blocks of a window over the lists; where nothing is expected to be unfinished (the
    // finish-in-place form) a wave keeps its column: the jumps cost the all-exterior tile 3 of its 23 us
    // (profiles/r03/light_path_ab.txt).
    // (row strips wrap nothing: the column jump below counts 8x8 block columns, so it stays off with them -- strip implies
    // inline_todo today; the second condition keeps that true should the two ever be decoupled)
    s.col_period = (inline_todo || strip) ? 0u : ctx->opt[MBK_OPT_SCAN_COL_PERIOD];
    if (s.xcd_map) s.col_jump = 32u * (((a.blocks_x / 32u) * 5u / 16u) | 1u);
    else s.col_jump = std::max(1u, a.blocks_x * 5u / 16u);
    if (s.col_jump >= a.blocks_x) s.col_jump = 0u, s.col_period = 0u;
    s.fast_bx_end = a.ncols / (strip ? 64u : 8u);
    // block rows (strips: rows) whose imaginary coordinates all come from the regular formula (the asm computes them that way)
    const uint32_t im_n = a.im.n - (axis_end_is_regular(a.im) ? 0u : 1u);
    s.fast_by_end = std::min(a.nrows / region_h, im_n > a.row0 ? (im_n - a.row0) / region_h : 0u);
    s.qtab = quant_table4(a.mrd, a.bytes != nullptr);
    s.long_groups = ctx->opt[MBK_OPT_GROUP_STEPS] >= 16u ? 1u : 0u;   // (the scan path has no 32-step form: 32 means 16)
    set_window_facts(a, f32);
    if (inline_todo) {
        // one launch, no lists, no scratch: a block the light path cannot finish is finished where it is found
        const bool stats = fuse != nullptr && fuse->slots != nullptr && (a.bytes || !fuse->counts_unwanted);
        if (stats) {
            a.stats = fuse->slots;
            if (fuse->counts_unwanted) a.counts = nullptr;
        }
        hipLaunchKernelGGL(pick_light_kernel<T>(cyc ? 2 : 1, stats, a.counts != nullptr, a.bytes != nullptr), dim3(w1), dim3(64), 0, stream, a, s);
        MBK_HIP(ctx, hipGetLastError());
        if (stats) fuse->fused = true;
        return MBK_OK;
    }

    // every list is fed by the waves with its index mod 64; a wave lists at most its own blocks
    const uint32_t qcap = ((w1 + mbk::kScanQueues - 1u) / mbk::kScanQueues) * ((nby + s.stride_by - 1u) / s.stride_by);
    StreamScratch *sc = nullptr;
    const int rc = acquire_scan_lists(ctx, stream, qcap, probe_share, s, &sc);
    if (rc != MBK_OK) return rc;
    hipLaunchKernelGGL(pick_light_kernel<T>(0, false, a.counts != nullptr, a.bytes != nullptr), dim3(w1), dim3(64), 0, stream, a, s);
    const uint32_t lds2 = ctx->wave_limit_lds[ctx->opt[MBK_OPT_WAVE_LIMIT] & 7u];
    hipLaunchKernelGGL(pick_todo_kernel<T>(cyc), dim3(mbk::kScanQueues * s.ranks2), dim3(64), lds2, stream, a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sc->cursors_dirty = true;
        return fail(ctx, MBK_ERR_HIP, std::string("scan launch: ") + hipGetErrorString(e));
    }
    return MBK_OK;
}

// The axes and the window of `v` in a kernel's arguments (TileArgs, DistanceArgs: the same fields)
template <typename Args>
static void fill_window(Args &a, const mbk_view *v)
{
    a.re = make_axis(v->start_r, v->range_r, v->width);
    a.im = make_axis(v->start_i, v->range_i, v->height);
    a.col0 = v->col0;
    a.row0 = v->row0;
    a.ncols = v->ncols;
    a.nrows = v->nrows;
}

static int launch_tile(mbk_ctx *ctx, const mbk_view *v, uint32_t mrd, uint32_t flags,
                       int32_t *d_counts, uint8_t *d_bytes, hipStream_t stream, double *d_smooth = nullptr, FuseStats *fuse = nullptr)
{
    if (flags & MBK_DEEP_BLA) return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_BLA is a flag of the deep view calls");
    if (flags & MBK_DEEP_XBLA) return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA is a flag of the extended-range deep view calls");
    if (fuse) fuse->fused = false;
    if (!ctx->capturing && stream != ctx->last_tile_stream) {   // (a capture runs nothing: no launch the shares could have felt)
        ctx->last_tile_stream = stream;
        ++ctx->stream_switches;
    }
    bool safe = false;
    const bool f32 = (flags & MBK_PRECISION_F32) != 0;
    int rc = validate_view(ctx, v, &safe, f32);
    if (rc != MBK_OK) return rc;
    if (mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    const bool wc = (flags & MBK_WANT_COUNTS) != 0, wb = (flags & MBK_WANT_BYTES) != 0;
    if (!wc && !wb && !d_smooth) return fail(ctx, MBK_ERR_INVALID, "flags select no output");
    if (wc && !d_counts) return fail(ctx, MBK_ERR_INVALID, "MBK_WANT_COUNTS with NULL counts pointer");
    if (wb && !d_bytes) return fail(ctx, MBK_ERR_INVALID, "MBK_WANT_BYTES with NULL bytes pointer");
    if (wb && mrd == 0) return fail(ctx, MBK_ERR_INVALID, "mrd == 0 has no quantised form (division by zero)");

    TileArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.out_pitch = v->ncols;
    a.out_col0 = 0;
    a.out_row0 = 0;
    a.mrd = (int32_t)mrd;
    a.quant_wide = (mrd >= (1u << 23)) ? 1u : 0u;
    a.quant_rcp = mrd ? 1.0 / (double)mrd : 0.0;
    a.perm_mul = 1u;
    a.exact_steps = ctx->opt[MBK_OPT_EXACT_STEPS];
    a.exact_steps_long = std::min(ctx->opt[MBK_OPT_EXACT_STEPS], ctx->opt[MBK_OPT_EXACT_LONG]);
    a.cyc_window = ctx->opt[MBK_OPT_CYCLE_WINDOW];
    a.order = nullptr;
    a.counts = wc ? d_counts : nullptr;
    a.bytes = wb ? d_bytes : nullptr;
    a.smooth = d_smooth;

    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if (d_smooth && (f32 || kernel == MBK_KERNEL_SIMPLE || kernel == MBK_KERNEL_REFILL))
        return fail(ctx, MBK_ERR_INVALID, "smooth colouring is implemented by the fp64 scan / asm / group kernels only");
    if (f32 && (kernel == MBK_KERNEL_SIMPLE || kernel == MBK_KERNEL_REFILL))
        return fail(ctx, MBK_ERR_INVALID, "MBK_PRECISION_F32 is implemented by the scan / asm / group kernels only");
    switch (kernel) {
        case MBK_KERNEL_DEFAULT:
        case MBK_KERNEL_SCAN: {
            // Default = a deterministic function of the window (round 3; rounds 1-2 followed the heavy share the
            // PREVIOUS launch on the stream had reported, which made a launch's time depend on history and sent every
            // tile after a change -- a real pyramid alternates -- to the wrong kernel).  window_heavy_share probes
            // 256 pixels of the window for the 4 steps the light pass runs.  With more than ~1 %
            // (MBK_OPT_HEAVY_SHARE) of them unfinished the tile is bound by the arithmetic of its heavy blocks and the
            // light ones ride along for free in "group" (cfg2: scan 597 us, group 568); below that "group" is bound
            // by its 0.27 ns per workgroup and its stores, and "scan" wins (all-exterior tile: 29 us against 71).
            // Launches under 16 k blocks take "group", which for them is a single kernel in image order (cfg1: 20
            // us, scan 24).  heavy_share = 0 forces "group", 65536 forces "scan".
            // Inside a capture (mbk.h "Graph capture") the two-pass form of "scan" is never taken: its two cursor sets alternate
            // per ENQUEUE -- pass 1 of launch L clears the set of launch L + 1 -- so a capture, which enqueues without running,
            // would leave the next launch a set nobody cleared, and a replay would append behind its own tails; the size of
            // its pass 2 comes from a hint the host reads at enqueue time.  The selector "scan" is refused there, and the
            // default takes "group" where it would take the two-pass form (every selector stores the same results) -- behind a
            // dispatch list if the stream's lists are large enough, in image order otherwise: the warm call, which took
            // "scan", was no occasion to grow them.  The finish-in-place form (one kernel, no scratch) stays the default's.
            if (ctx->capturing && kernel == MBK_KERNEL_SCAN)
                return refuse_capture(ctx, "MBK_KERNEL_SCAN is not served inside a capture: take the default selector, group or asm");
            if (kernel == MBK_KERNEL_DEFAULT && (uint64_t)((a.ncols + 7u) / 8u) * ((a.nrows + 7u) / 8u) < 16384u)
                return launch_blocks(ctx, a, MBK_KERNEL_GROUP, safe, f32, stream);
            const double share = window_heavy_share(ctx, a);
            if (kernel == MBK_KERNEL_DEFAULT &&
                (share * 65536.0 > (double)ctx->opt[MBK_OPT_HEAVY_SHARE] || ctx->opt[MBK_OPT_HEAVY_SHARE] == 0u))
                return launch_blocks(ctx, a, MBK_KERNEL_GROUP, safe, f32, stream, fuse);
            if (ctx->capturing && !(share == 0.0 && ctx->opt[MBK_OPT_SCAN_INLINE] != 0u))
                return launch_blocks(ctx, a, MBK_KERNEL_GROUP, safe, f32, stream, nullptr, true);
            return f32 ? launch_scan_t<float>(ctx, a, safe, stream, share, fuse) : launch_scan_t<double>(ctx, a, safe, stream, share, fuse);
        }
        case MBK_KERNEL_GROUP:
        case MBK_KERNEL_ASM:
            return launch_blocks(ctx, a, kernel, safe, f32, stream, fuse);
        case MBK_KERNEL_REFILL:
            return launch_refill(ctx, a, safe, stream);
        case MBK_KERNEL_SIMPLE: {
            a.blocks_x = (v->ncols + 31u) / 32u;
            const uint32_t by = (v->nrows + 7u) / 8u;
            const dim3 grid(a.blocks_x * by), block(256);
            hipLaunchKernelGGL(mbk::tile_simple_kernel<false>, grid, block, 0, stream, a);
            break;
        }
        default:
            return fail(ctx, MBK_ERR_INVALID, "unknown MBK_KERNEL_* selector");
    }
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// Grow the device buffer `p` of capacity `cap` (in the caller's unit: pixels, bytes) to `need` of them, which take `bytes`
// bytes.  Free, clear pointer and capacity, allocate, set the capacity -- in this order, so that a failed hipMalloc leaves
// no dangling pointer with a stale capacity.  (hipFree waits for the launches that may still read the old buffer.)
template <typename T>
static int grow(mbk_ctx *ctx, T *&p, size_t &cap, size_t need, size_t bytes)
{
    if (need <= cap) return MBK_OK;
    if (ctx->capturing) return refuse_capture(ctx, "the stream's scratch must grow for this call: make the same call, or a larger one, once outside the capture");
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    MBK_HIP(ctx, hipMalloc((void **)&p, bytes));
    cap = need;
    return MBK_OK;
}

// counts and bytes of a slot, both under cap_px: it is zero until both exist
static int ensure_buffers(mbk_ctx *ctx, Slot &sl, size_t px)
{
    if (px <= sl.cap_px) return MBK_OK;
    size_t cap_counts = 0, cap_bytes = 0;
    sl.cap_px = 0;
    int rc = grow(ctx, sl.d_counts, cap_counts, px, px * sizeof(int32_t));
    if (rc == MBK_OK) rc = grow(ctx, sl.d_bytes, cap_bytes, px, px);
    if (rc == MBK_OK) sl.cap_px = px;
    return rc;
}

// clear = false: the partial results were zeroed earlier on this stream and a tile kernel has already added its fused
// share (pixel-iterations, never-escaped count); this pass then reads the bytes only.
static int launch_reduce(mbk_ctx *ctx, ReduceSlot *d_red, ReduceSlot *h_red, const int32_t *d_counts, const uint8_t *d_bytes,
                         uint64_t n, uint32_t mrd, hipStream_t stream, bool clear = true)
{
    if (clear) MBK_HIP(ctx, hipMemsetAsync(d_red, 0, sizeof(ReduceSlot) * mbk::kReduceSlots, stream));
    if (!d_counts && !d_bytes) {   // everything was fused into the tile kernel
        MBK_HIP(ctx, hipMemcpyAsync(h_red, d_red, sizeof(ReduceSlot) * mbk::kReduceSlots, hipMemcpyDeviceToHost, stream));
        return MBK_OK;
    }
    const bool vec = n >= 1024u && ((uintptr_t)d_counts & 15u) == 0u && ((uintptr_t)d_bytes & 3u) == 0u;
    uint64_t blocks = ((vec ? n / 4u : n) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks == 0) blocks = 1;
    // four pixels per lane and trip; the scalar kernel serves unaligned sub-buffers and tiny inputs
    if (vec && d_counts && d_bytes)
        hipLaunchKernelGGL((mbk::reduce_vec_kernel<true, true>), dim3((uint32_t)blocks), dim3(256), 0, stream, d_counts,
                           d_bytes, n, mrd, d_red);
    else if (vec && d_counts)
        hipLaunchKernelGGL((mbk::reduce_vec_kernel<true, false>), dim3((uint32_t)blocks), dim3(256), 0, stream, d_counts,
                           d_bytes, n, mrd, d_red);
    else if (vec && d_bytes)
        hipLaunchKernelGGL((mbk::reduce_vec_kernel<false, true>), dim3((uint32_t)blocks), dim3(256), 0, stream, d_counts,
                           d_bytes, n, mrd, d_red);
    else
        hipLaunchKernelGGL(mbk::reduce_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, d_counts,
                           d_bytes, n, mrd, d_red);
    MBK_HIP(ctx, hipGetLastError());
    MBK_HIP(ctx, hipMemcpyAsync(h_red, d_red, sizeof(ReduceSlot) * mbk::kReduceSlots, hipMemcpyDeviceToHost, stream));
    return MBK_OK;
}
static int launch_reduce(mbk_ctx *ctx, Slot &sl, const int32_t *d_counts, const uint8_t *d_bytes, uint64_t n,
                         uint32_t mrd, hipStream_t stream, bool clear = true)
{
    return launch_reduce(ctx, sl.d_red, sl.h_red, d_counts, d_bytes, n, mrd, stream, clear);
}

// the partial results of a finished reduction (the stream has been synchronised), added up
static ReduceOut reduce_total(const ReduceSlot *h_red)
{
    ReduceOut t = {};
    for (uint32_t k = 0; k < mbk::kReduceSlots; ++k) {
        const ReduceOut &r = h_red[k].r;
        t.pixel_iterations += r.pixel_iterations;
        t.never_pixels += r.never_pixels;
        t.run_starts += r.run_starts;
        t.any_byte_not_zero |= r.any_byte_not_zero;
        t.any_byte_not_one |= r.any_byte_not_one;
    }
    return t;
}

static ReduceOut reduce_total(const Slot &sl) { return reduce_total(sl.h_red); }

static void fill_stats_from_reduce(const ReduceSlot *h_red, mbk_stats *s, bool have_bytes)
{
    const ReduceOut t = reduce_total(h_red);
    s->pixel_iterations = t.pixel_iterations;
    s->never_pixels = t.never_pixels;
    s->all_bytes_zero = have_bytes && t.any_byte_not_zero == 0 ? 1u : 0u;
    s->all_bytes_one = have_bytes && t.any_byte_not_one == 0 ? 1u : 0u;
    s->rle_runs = have_bytes ? t.run_starts : 0ull;
}

// The statistics of a finished slot (its stream has been synchronised): the times between its events and, if `reduced`,
// the totals of its reduction scratch.
static int slot_stats(mbk_ctx *ctx, const Slot &sl, mbk_stats *stats, bool have_bytes, bool reduced = true)
{
    std::memset(stats, 0, sizeof(*stats));
    MBK_HIP(ctx, hipEventElapsedTime(&stats->kernel_ms, sl.ev_k0, sl.ev_k1));
    MBK_HIP(ctx, hipEventElapsedTime(&stats->d2h_ms, sl.ev_c0, sl.ev_c1));
    if (reduced) fill_stats_from_reduce(sl.h_red, stats, have_bytes);
    return MBK_OK;
}

// ---- the synchronous calls (mbk_*_compute*, DESIGN.md "A synchronous call") ------------------------------------------
// They run on slot 0 -- its stream, buffers, events and reduction scratch -- and are made of three parts: the entry point's
// own refusals and sync_begin; an enqueue step that returns a status and never waits; sync_end on that status.

static int sync_begin(mbk_ctx *ctx)
{
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->s[0].busy) return fail(ctx, MBK_ERR_INVALID, "slot 0 has a tile in flight: call mbk_wait first");
    return MBK_OK;
}

// rc: what the enqueue step returned.  A failure may have left work queued that still writes into the slot's and the ctx'
// buffers: the stream is drained before the status goes back (the error text is already in place).  Otherwise wait and
// fill `stats` (may be NULL); have_bytes / reduced as for slot_stats.
static int sync_end(mbk_ctx *ctx, int rc, mbk_stats *stats, bool have_bytes, bool reduced = true)
{
    Slot &sl = ctx->s[0];
    if (rc != MBK_OK) {
        (void)hipStreamSynchronize(sl.stream);
        return rc;
    }
    MBK_HIP(ctx, hipStreamSynchronize(sl.stream));
    return stats ? slot_stats(ctx, sl, stats, have_bytes, reduced) : MBK_OK;
}

// The calls that return one binary64 value per pixel (smooth, distance, deep distance, interior) between sync_begin and the return:
// launch(d_counts, d_values, stream) enqueues the kernels that write both.  with_tail (interior views): the device values are
// followed by px int32 (the periods, at d_values + px), which the launch writes too; they go to h_tail, and h_values and h_tail
// may each be NULL.  per_px (atom periods and Newton seeds): that many binary64 values per pixel, the tail after all of them.
// h_more (normals with distance estimates; not with a tail): px more binary64 values follow the per_px * px on the device, at
// d_values + per_px * px, which the launch writes too; they go to h_more.  h_more2 (deep normals: nu in h_more, rel here): px
// further values behind those, at d_values + (per_px + 1) * px whether or not h_more is given.  more_per_px (the stripe state:
// 32 bytes per pixel; not with h_more2): that many binary64 values per pixel in h_more.
template <typename Launch>
static int compute_values(mbk_ctx *ctx, size_t px, uint32_t mrd, int32_t *h_counts, double *h_values, mbk_stats *stats, Launch launch,
                          bool with_tail = false, int32_t *h_tail = nullptr, size_t per_px = 1u, double *h_more = nullptr,
                          double *h_more2 = nullptr, size_t more_per_px = 1u)
{
    Slot &sl = ctx->s[0];
    auto enqueue = [&]() -> int {
        int rc = ensure_buffers(ctx, sl, px);
        if (rc != MBK_OK) return rc;
        const size_t vals = per_px * px;
        const size_t cap = with_tail ? vals + (px + 1u) / 2u : (h_more2 ? vals + 2u * px : (h_more ? vals + more_per_px * px : vals));   // (in binary64 values)
        rc = grow(ctx, ctx->d_smooth, ctx->smooth_cap_px, cap, cap * sizeof(double));
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
        rc = launch(sl.d_counts, ctx->d_smooth, sl.stream);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_k1, sl.stream));
        rc = launch_reduce(ctx, sl, sl.d_counts, nullptr, px, mrd, sl.stream);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        if (h_values) MBK_HIP(ctx, hipMemcpyAsync(h_values, ctx->d_smooth, vals * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
        if (h_tail) MBK_HIP(ctx, hipMemcpyAsync(h_tail, ctx->d_smooth + vals, px * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
        if (h_more) MBK_HIP(ctx, hipMemcpyAsync(h_more, ctx->d_smooth + vals, more_per_px * px * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
        if (h_more2) MBK_HIP(ctx, hipMemcpyAsync(h_more2, ctx->d_smooth + vals + px, px * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
        if (h_counts) MBK_HIP(ctx, hipMemcpyAsync(h_counts, sl.d_counts, px * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        ctx->last_px = 0;   // (no bytes on the device: mbk_serialize_last has nothing to read)
        return MBK_OK;
    };
    return sync_end(ctx, enqueue(), stats, false);
}

// The first pass of a two-pass launch (distance estimates, normals, stripe averages, interior views) of px pixels on `stream`:
// count_launch(counts) has the escape kernels write the counts the second pass runs on -- the caller's, or the stream's scratch
// when the caller wants none; *d_counts is where they are.
template <typename CountLaunch>
static int launch_count_pass(mbk_ctx *ctx, size_t px, hipStream_t stream, int32_t **d_counts, CountLaunch count_launch)
{
    if (!*d_counts) {
        StreamScratch *sc = nullptr;
        int rc = get_scratch(ctx, stream, &sc);
        if (rc == MBK_OK) rc = grow(ctx, sc->d_dist_counts, sc->dist_cap_px, px, px * sizeof(int32_t));
        if (rc != MBK_OK) return rc;
        *d_counts = sc->d_dist_counts;
    }
    return count_launch(*d_counts);
}

// MBK_WANT_* flags need the pointers they fill
static int check_wanted(mbk_ctx *ctx, uint32_t flags, const void *counts, const void *bytes)
{
    if ((flags & MBK_WANT_COUNTS) && !counts) return fail(ctx, MBK_ERR_INVALID, "MBK_WANT_COUNTS with NULL counts pointer");
    if ((flags & MBK_WANT_BYTES) && !bytes) return fail(ctx, MBK_ERR_INVALID, "MBK_WANT_BYTES with NULL bytes pointer");
    return MBK_OK;
}

// enqueue kernel + reduction + D2H of a checked view on a slot's stream (no host synchronisation): the enqueue step of the deep
// and the Julia views, synchronous (h_smooth may be given) and slot forms alike.  launch(d_counts, d_bytes, d_smooth, stream)
// enqueues the kernel; counts always go to the device, they feed the statistics.
template <typename Launch>
static int view_enqueue(mbk_ctx *ctx, Slot &sl, size_t px, uint32_t mrd, uint32_t flags, int32_t *h_counts, uint8_t *h_bytes,
                        double *h_smooth, Launch launch)
{
    const bool wc = (flags & MBK_WANT_COUNTS) != 0, wb = (flags & MBK_WANT_BYTES) != 0;
    int rc = ensure_buffers(ctx, sl, px);
    if (rc == MBK_OK && h_smooth) rc = grow(ctx, ctx->d_smooth, ctx->smooth_cap_px, px, px * sizeof(double));
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
    rc = launch(sl.d_counts, wb ? sl.d_bytes : nullptr, h_smooth ? ctx->d_smooth : nullptr, sl.stream);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipEventRecord(sl.ev_k1, sl.stream));
    rc = launch_reduce(ctx, sl, sl.d_counts, wb ? sl.d_bytes : nullptr, px, mrd, sl.stream);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
    if (wc) MBK_HIP(ctx, hipMemcpyAsync(h_counts, sl.d_counts, px * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    if (wb) MBK_HIP(ctx, hipMemcpyAsync(h_bytes, sl.d_bytes, px, hipMemcpyDeviceToHost, sl.stream));
    if (h_smooth) MBK_HIP(ctx, hipMemcpyAsync(h_smooth, ctx->d_smooth, px * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
    MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
    if (&sl == &ctx->s[0]) ctx->last_px = wb ? px : 0;
    return MBK_OK;
}

// The slot form of such a view behind its own refusals: slot range, output selection, pointers, a free slot; then the enqueue
// step and the slot's bookkeeping.
template <typename Launch>
static int view_submit(mbk_ctx *ctx, int slot, size_t px, uint32_t mrd, uint32_t flags, int32_t *h_counts, uint8_t *h_bytes, Launch launch)
{
    if (slot < 0 || slot >= MBK_SLOTS) return fail(ctx, MBK_ERR_INVALID, "slot out of range");
    if (!(flags & (MBK_WANT_COUNTS | MBK_WANT_BYTES))) return fail(ctx, MBK_ERR_INVALID, "flags select no output");
    int rc = check_wanted(ctx, flags, h_counts, h_bytes);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    Slot &sl = ctx->s[slot];
    if (sl.busy) return fail(ctx, MBK_ERR_INVALID, "slot still has a tile in flight: call mbk_wait first");
    rc = view_enqueue(ctx, sl, px, mrd, flags, h_counts, h_bytes, nullptr, launch);
    if (rc != MBK_OK) return rc;
    sl.immediate = false;
    sl.lazy_h_bytes = nullptr;
    sl.busy = true;
    sl.with_bytes = (flags & MBK_WANT_BYTES) != 0;
    return MBK_OK;
}

// The synchronous form behind its own refusals: output selection, pointers; sync_begin, the enqueue step, sync_end.
template <typename Launch>
static int view_compute(mbk_ctx *ctx, size_t px, uint32_t mrd, uint32_t flags, int32_t *h_counts, uint8_t *h_bytes, double *h_smooth,
                        mbk_stats *stats, Launch launch)
{
    if (!(flags & (MBK_WANT_COUNTS | MBK_WANT_BYTES)) && !h_smooth) return fail(ctx, MBK_ERR_INVALID, "flags and h_smooth select no output");
    int rc = check_wanted(ctx, flags, h_counts, h_bytes);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    return sync_end(ctx, view_enqueue(ctx, ctx->s[0], px, mrd, flags, h_counts, h_bytes, h_smooth, launch), stats, (flags & MBK_WANT_BYTES) != 0);
}

// ---- the four kinds of view behind one type (DESIGN.md "One target, four kinds of view") --------------------------------

struct Geometry { uint32_t width, height, col0, row0, ncols, nrows; };

// What a count call, a render or a histogram works on: a plain view, the Julia set of (c_r, c_i) on a view, a deep view or an
// extended-range deep view on `orbit`.  The view struct of the kind is held by value, so a target outlives the caller's struct
// and a piece of it (target_samples) is a target like any other.  A NULL view leaves has_view false and the kind in place:
// the refusals of a NULL view stand at a different place in each kind's order (target_check).
struct Target {
    enum Kind { kPlain, kJulia, kDeep, kWide } kind;
    bool has_view;
    Geometry g;                    // the geometry of the view of `kind`, whichever struct holds it
    mbk_view view;                 // kPlain, kJulia
    mbk_deep_view deep;            // kDeep
    mbk_deep_xview wide;           // kWide
    const mbk_deep_orbit *orbit;   // kDeep, kWide
    double c_r, c_i;               // kJulia
};

template <typename V>
static Target make_target(Target::Kind kind, const V *v, V Target::*held, const mbk_deep_orbit *orbit = nullptr, double c_r = 0.0,
                          double c_i = 0.0)
{
    Target t = {};
    t.kind = kind;
    t.orbit = orbit;
    t.c_r = c_r;
    t.c_i = c_i;
    if (v) {
        t.has_view = true;
        t.*held = *v;
        t.g = Geometry{v->width, v->height, v->col0, v->row0, v->ncols, v->nrows};
    }
    return t;
}
static Target view_target(const mbk_view *v) { return make_target(Target::kPlain, v, &Target::view); }
static Target julia_target(const mbk_view *v, double c_r, double c_i) { return make_target(Target::kJulia, v, &Target::view, nullptr, c_r, c_i); }
static Target deep_target(const mbk_deep_orbit *orbit, const mbk_deep_view *v) { return make_target(Target::kDeep, v, &Target::deep, orbit); }
static Target wide_target(const mbk_deep_orbit *orbit, const mbk_deep_xview *v) { return make_target(Target::kWide, v, &Target::wide, orbit); }

template <typename V>
static void set_geometry(V &v, const Geometry &g)
{
    v.width = g.width;
    v.height = g.height;
    v.col0 = g.col0;
    v.row0 = g.row0;
    v.ncols = g.ncols;
    v.nrows = g.nrows;
}

// The samples of the piece (col0, row0, ncols, nrows) of the OUTPUT window of `t` at supersample s: the same rectangle or
// spans at s times the width and height.
static Target target_samples(const Target &t, uint32_t s, uint32_t col0, uint32_t row0, uint32_t ncols, uint32_t nrows)
{
    Target p = t;
    p.g = Geometry{t.g.width * s, t.g.height * s, col0 * s, row0 * s, ncols * s, nrows * s};
    switch (t.kind) {
        case Target::kWide: set_geometry(p.wide, p.g); break;
        case Target::kDeep: set_geometry(p.deep, p.g); break;
        case Target::kJulia:
        case Target::kPlain: set_geometry(p.view, p.g); break;
    }
    return p;
}

// Bands (renders, histograms, density views): rows of a window whose samples fit MBK_RENDER_BAND_BYTES of scratch at
// bytes_per_px bytes per pixel, and pieces of columns where one row's do not.  max_rows: a cap on the rows of a band, or 0.
struct BandPlan {
    uint32_t ncols, nrows, tile_cols, band_rows;
    size_t cap_px() const { return (size_t)tile_cols * band_rows; }
};

static BandPlan band_plan(uint32_t ncols, uint32_t nrows, uint64_t bytes_per_px, uint32_t max_rows = 0u)
{
    const uint64_t budget = MBK_RENDER_BAND_BYTES - 1024u;   // (the parts of the scratch start on 256-byte lines)
    BandPlan p = {ncols, nrows, ncols, 1u};
    if ((uint64_t)ncols * bytes_per_px <= budget)
        p.band_rows = (uint32_t)std::min<uint64_t>(nrows, budget / ((uint64_t)ncols * bytes_per_px));
    else
        p.tile_cols = (uint32_t)(budget / bytes_per_px);
    if (max_rows) p.band_rows = std::min(p.band_rows, max_rows);
    return p;
}

// piece(r, c, nr, nc, is_last) enqueues the piece at (r, c) of the window on `stream`, its counts -- samples_per_px of them per
// pixel -- at d_counts.  stat: the slot whose reduction scratch adds up the statistics of the counts and whose ev_k1 marks the
// last piece's last kernel (the synchronous forms), or NULL.
template <typename Piece>
static int for_each_band(mbk_ctx *ctx, const BandPlan &p, const int32_t *d_counts, uint64_t samples_per_px, uint32_t mrd,
                         hipStream_t stream, Slot *stat, Piece piece)
{
    for (uint32_t r = 0; r < p.nrows; r += p.band_rows) {
        const uint32_t nr = std::min(p.band_rows, p.nrows - r);
        for (uint32_t c = 0; c < p.ncols; c += p.tile_cols) {
            const uint32_t nc = std::min(p.tile_cols, p.ncols - c);
            const bool is_last = r + nr == p.nrows && c + nc == p.ncols;
            int rc = piece(r, c, nr, nc, is_last);
            if (rc != MBK_OK) return rc;
            if (stat) {
                if (is_last) MBK_HIP(ctx, hipEventRecord(stat->ev_k1, stream));
                rc = launch_reduce(ctx, stat->d_red, stat->h_red, d_counts, nullptr, (uint64_t)nc * nr * samples_per_px, mrd, stream, false);
                if (rc != MBK_OK) return rc;
            }
        }
    }
    return MBK_OK;
}

// ---- what deep and extended-range deep views share: mbk_deep_view and mbk_deep_xview, DeepArgs and DeepWideArgs name these
// fields the same ----

static double deep_step(double range, uint32_t n)
{
    if (n <= 1u) return 0.0;
    volatile double s = range / (double)(n - 1u);
    return s;
}

// dc of sample k of an axis of n samples over `range`: fl(fl(k - (n - 1) / 2) * step), as the kernels form it
static double deep_dc(uint32_t k, uint32_t n, double range)
{
    volatile double dc = ((double)k - (double)(n - 1u) * 0.5) * deep_step(range, n);
    return dc;
}

// The common front of the one-pixel host twins, after the view's own checks: the pixel must lie in the view; its dc.
struct PixelDc {
    int rc;
    double r, i;
};

template <typename V>
static PixelDc pixel_dc(const V *view, uint32_t col, uint32_t row)
{
    if (col >= view->width || row >= view->height) return PixelDc{fail(nullptr, MBK_ERR_INVALID, "pixel outside the view"), 0.0, 0.0};
    return PixelDc{MBK_OK, deep_dc(col, view->width, view->range_r), deep_dc(row, view->height, view->range_i)};
}

template <typename V>
static bool deep_ranges_within(const V *v, double lo)
{
    for (double r : {v->range_r, v->range_i})
        if (!std::isfinite(r) || !(r >= lo) || !(r <= 4.0)) return false;
    return true;
}

// The checks of a deep view of either kind, in the order the calls report them: the pointers, the kind's flag rules
// (flag_rules()), the geometry, the kind's ranges (range_rules()), mrd.
template <typename V, typename FlagRules, typename RangeRules>
static int validate_deep_view(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const V *v, uint32_t mrd, uint32_t flags, FlagRules flag_rules,
                              RangeRules range_rules)
{
    if (!orbit) return fail(ctx, MBK_ERR_INVALID, "orbit is NULL");
    if (!v) return fail(ctx, MBK_ERR_INVALID, "view is NULL");
    int rc = flag_rules();
    if (rc != MBK_OK) return rc;
    if (v->width == 0 || v->height == 0) return fail(ctx, MBK_ERR_INVALID, "empty view");
    if (v->ncols == 0 || v->nrows == 0) return fail(ctx, MBK_ERR_INVALID, "empty window");
    if ((uint64_t)v->col0 + v->ncols > v->width || (uint64_t)v->row0 + v->nrows > v->height)
        return fail(ctx, MBK_ERR_INVALID, "window exceeds the view");
    if ((uint64_t)v->ncols * v->nrows > (1ull << 31)) return fail(ctx, MBK_ERR_INVALID, "window larger than 2^31 pixels");
    rc = range_rules();
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(ctx, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    if ((flags & MBK_WANT_BYTES) && mrd == 0) return fail(ctx, MBK_ERR_INVALID, "mrd == 0 has no quantised form (division by zero)");
    return MBK_OK;
}

// the view's geometry and window and mrd in a deep kernel's arguments
template <typename Args, typename V>
static void fill_deep_window(Args &a, const V *v, uint32_t mrd)
{
    a.half_r = (double)(v->width - 1u) * 0.5;
    a.half_i = (double)(v->height - 1u) * 0.5;
    a.step_r = deep_step(v->range_r, v->width);
    a.step_i = deep_step(v->range_i, v->height);
    a.col0 = v->col0;
    a.row0 = v->row0;
    a.ncols = v->ncols;
    a.nrows = v->nrows;
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.mrd = (int32_t)mrd;
}

// the three outputs (each may be null) and the quantiser of the bytes (mbk_kernels.h: quantise) in a kernel's arguments
template <typename Args>
static void fill_outputs(Args &a, uint32_t mrd, int32_t *d_counts, uint8_t *d_bytes, double *d_smooth)
{
    a.quant_wide = (mrd >= (1u << 23)) ? 1u : 0u;
    a.quant_rcp = mrd ? 1.0 / (double)mrd : 0.0;
    a.counts = d_counts;
    a.bytes = d_bytes;
    a.smooth = d_smooth;
}

// one 64-lane workgroup per 8 x 8 block of the window in `a` (blocks_x set)
template <typename Args>
static dim3 block_grid(const Args &a) { return dim3(a.blocks_x * ((a.nrows + 7u) / 8u)); }

// ------------------------------------- C ABI ---------------------------------------------------

extern "C" {

int mbk_abi_version(void) { return MBK_ABI_VERSION; }

int mbk_device_count(int *count)
{
    if (!count) return fail(nullptr, MBK_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(nullptr, MBK_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return MBK_OK;
}

int mbk_create(int device, mbk_ctx **out)
{
    if (!out) return fail(nullptr, MBK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, MBK_ERR_NO_DEVICE,
                    std::string("no HIP device visible (") + hipGetErrorString(e) +
                        "); libmbk_hip has no CPU fallback");
    if (device < 0 || device >= n) return fail(nullptr, MBK_ERR_NO_DEVICE, "device index out of range");
    mbk_ctx *ctx = new (std::nothrow) mbk_ctx();
    if (!ctx) return fail(nullptr, MBK_ERR_NOMEM, "out of host memory");
    ctx->device = device;
    static const uint32_t kDefaults[MBK_OPT_COUNT_] = {
        /* ORDER */ 3u, /* WAVES_PER_WG */ 1u, /* GROUP_STEPS */ 16u, /* EXACT_STEPS */ 8u, /* PROBE_STEPS */ 32u,
        /* SCAN_WAVES */ 8u, /* SCAN_XCD_MAP */ 1u, /* SCAN_COL_PERIOD */ 4u, /* HEAVY_SHARE */ 655u,
        /* RF_LIVEMIN */ 48u, /* RF_PATIENCE */ 256u, /* RF_BATCH */ 1u, /* RF_WAVES */ 8u, /* CYCLE_DETECT */ 1u,
        /* PROBE_MID */ 65537u, /* PREPASS_OVERLAP */ 1u, /* EXACT_LONG */ 0u, /* SCAN_INLINE */ 1u, /* WAVE_LIMIT */ 0u,
        /* UNITS_MIN_LIGHT */ 32768u, /* XCD_BALANCE */ 0u, /* M_LATE */ 8u, /* H_SETTLED */ 6u, /* CLASSIFY_WG */ 1024u,
        /* SCAN_STRIP */ 1u, /* CYCLE_WINDOW */ 32u, /* SPILL_FIRST */ 256u, /* SPILL_LANES */ 16u, /* SPILL_MIN_MRD */ 2048u, /* SPILL_MIN_BLOCKS */ 19u, /* SPILL_CYC_SHIFT */ 5u,
        /* SURE_INTERIOR */ 1u};
    std::memcpy(ctx->opt, kDefaults, sizeof(kDefaults));
#define MBK_CREATE_HIP(call)                                                        \
    do {                                                                            \
        hipError_t e2_ = (call);                                                    \
        if (e2_ != hipSuccess) {                                                    \
            fail(nullptr, MBK_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e2_)); \
            mbk_destroy(ctx);                                                       \
            return MBK_ERR_HIP;                                                     \
        }                                                                           \
    } while (0)
    MBK_CREATE_HIP(hipSetDevice(device));
    MBK_CREATE_HIP(hipGetDeviceProperties(&ctx->prop, device));
    if (std::strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0) {
        fail(nullptr, MBK_ERR_NO_DEVICE,
             std::string("device is ") + ctx->prop.gcnArchName + ", this library is built for gfx950 only");
        mbk_destroy(ctx);
        return MBK_ERR_NO_DEVICE;
    }
    for (Slot &sl : ctx->s) {
        MBK_CREATE_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        MBK_CREATE_HIP(hipEventCreate(&sl.ev_k0));
        MBK_CREATE_HIP(hipEventCreate(&sl.ev_k1));
        MBK_CREATE_HIP(hipEventCreate(&sl.ev_c0));
        MBK_CREATE_HIP(hipEventCreate(&sl.ev_c1));
        MBK_CREATE_HIP(hipMalloc((void **)&sl.d_red, sizeof(ReduceSlot) * mbk::kReduceSlots));
        MBK_CREATE_HIP(hipHostMalloc((void **)&sl.h_red, sizeof(ReduceSlot) * mbk::kReduceSlots, hipHostMallocDefault));
    }
    {
        const void *fns[2][2] = {{(const void *)mbk::tile_light_kernel<double, true, true>, (const void *)mbk::tile_todo_kernel<double>},
                                 {(const void *)mbk::tile_light_kernel<float, true, true>, (const void *)mbk::tile_todo_kernel<float>}};
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < 2; ++k) {
                int n = 0;
                MBK_CREATE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fns[f][k], 64, 0));
                ctx->scan_occ[f][k] = n > 0 ? n : 1;
            }
        // the finish-in-place launch is one of several instantiations (outputs x cycle test x fused statistics) with
        // their own register counts: size the persistent grid for the least resident of them, or a launch whose
        // instantiation holds fewer waves than assumed would run a second dispatch round
        const void *fi[2][6] = {{(const void *)mbk::tile_light_kernel<double, true, true, 2>, (const void *)mbk::tile_light_kernel<double, true, true, 1>,
                                 (const void *)mbk::tile_light_kernel<double, true, true, 2, true>, (const void *)mbk::tile_light_kernel<double, false, true, 2, true>,
                                 (const void *)mbk::tile_light_kernel<double, true, false, 2, true>, (const void *)mbk::tile_light_kernel<double, true, false, 1>},
                                {(const void *)mbk::tile_light_kernel<float, true, true, 2>, (const void *)mbk::tile_light_kernel<float, true, true, 1>,
                                 (const void *)mbk::tile_light_kernel<float, true, true, 2, true>, (const void *)mbk::tile_light_kernel<float, false, true, 2, true>,
                                 (const void *)mbk::tile_light_kernel<float, true, false, 2, true>, (const void *)mbk::tile_light_kernel<float, true, false, 1>}};
        for (int f = 0; f < 2; ++f) {
            int least = 0;
            for (int k = 0; k < 6; ++k) {
                int n = 0;
                MBK_CREATE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fi[f][k], 64, 0));
                n = n > 0 ? n : 1;
                least = (k == 0 || n < least) ? n : least;
            }
            ctx->scan_occ_inline[f] = least;
        }
    }
    {
        // MBK_OPT_WAVE_LIMIT: the smallest dynamic-LDS size per workgroup at which the occupancy calculator admits no more
        // than 4 k single-wave workgroups per CU (binary search on the runtime's own answer, no LDS granule assumed)
        const void *fn = (const void *)mbk::tile_asm_kernel<double, true, 16, false>;
        for (int k = 1; k <= 7; ++k) {
            uint32_t lo = 0, hi = 65536;   // occ(lo) > 4k >= occ(hi)
            int n = 0;
            MBK_CREATE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 64, hi));
            if (n > 4 * k) {
                ctx->wave_limit_lds[k] = hi;
                continue;
            }
            while (hi - lo > 64) {
                const uint32_t mid = (lo + hi) / 2;
                MBK_CREATE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 64, mid));
                if (n > 4 * k) lo = mid;
                else hi = mid;
            }
            ctx->wave_limit_lds[k] = hi;
        }
    }
#undef MBK_CREATE_HIP
    *out = ctx;
    return MBK_OK;
}

void mbk_destroy(mbk_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
    for (Slot &sl : ctx->s) {
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
        if (sl.d_counts) (void)hipFree(sl.d_counts);
        if (sl.d_bytes) (void)hipFree(sl.d_bytes);
        if (sl.d_red) (void)hipFree(sl.d_red);
        if (sl.h_red) (void)hipHostFree(sl.h_red);
        if (sl.ev_k0) (void)hipEventDestroy(sl.ev_k0);
        if (sl.ev_k1) (void)hipEventDestroy(sl.ev_k1);
        if (sl.ev_c0) (void)hipEventDestroy(sl.ev_c0);
        if (sl.ev_c1) (void)hipEventDestroy(sl.ev_c1);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
    }
    if (!ctx->scratch.empty() || !ctx->deep.empty()) (void)hipDeviceSynchronize();  // caller streams may still use them
    for (StreamScratch &sc : ctx->scratch) free_scratch(sc);
    for (mbk_ctx::DeepCopy &c : ctx->deep) free_deep_copy(c);
    if (ctx->d_rle) (void)hipFree(ctx->d_rle);
    if (ctx->d_smooth) (void)hipFree(ctx->d_smooth);
    if (ctx->d_rgba) (void)hipFree(ctx->d_rgba);
    if (ctx->d_hist) (void)hipFree(ctx->d_hist);
    if (ctx->d_density) (void)hipFree(ctx->d_density);
    if (ctx->d_density_stat) (void)hipFree(ctx->d_density_stat);
    delete ctx;
}

const char *mbk_last_error(const mbk_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int mbk_get_device_info(mbk_ctx *ctx, mbk_device_info *info)
{
    if (!ctx || !info) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    std::memset(info, 0, sizeof(*info));
    std::snprintf(info->name, sizeof(info->name), "%s", ctx->prop.name);
    std::snprintf(info->arch, sizeof(info->arch), "%s", ctx->prop.gcnArchName);
    info->compute_units = ctx->prop.multiProcessorCount;
    info->clock_mhz = ctx->prop.clockRate / 1000;
    info->wavefront_size = ctx->prop.warpSize;
    info->total_mem = ctx->prop.totalGlobalMem;
    return MBK_OK;
}

int mbk_device_pci_bus_id(mbk_ctx *ctx, char *buf, int len)
{
    if (!ctx || !buf || len < 16) return fail(ctx, MBK_ERR_INVALID, "buffer of at least 16 bytes needed");
    MBK_HIP(ctx, hipDeviceGetPCIBusId(buf, len, ctx->device));
    return MBK_OK;
}

int mbk_host_alloc(mbk_ctx *ctx, uint64_t bytes, void **out)
{
    if (!ctx || !out || bytes == 0) return fail(ctx, MBK_ERR_INVALID, "bad argument");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    MBK_HIP(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
    return MBK_OK;
}

int mbk_host_free(mbk_ctx *ctx, void *ptr)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!ptr) return MBK_OK;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    MBK_HIP(ctx, hipHostFree(ptr));
    return MBK_OK;
}

int mbk_datachunk_geometry(uint32_t level, uint32_t index_real, uint32_t index_imag,
                           double *start_r, double *start_i, double *range)
{
    if (!start_r || !start_i || !range) return fail(nullptr, MBK_ERR_INVALID, "NULL output pointer");
    if (level == 0) return fail(nullptr, MBK_ERR_INVALID, "level must be > 0 (DataChunk.cs:99-100)");
    if (index_real >= level || index_imag >= level)
        return fail(nullptr, MBK_ERR_INVALID, "chunk index must be < level (DataChunk.cs:102-106)");
    // WorkerCUDA.py:75-78: chunk_range = (MAX_AXIS - MIN_AXIS) / level; start = MIN_AXIS + chunk_range*index
    volatile double chunk_range = (2.0 - (-2.0)) / (double)level;
    volatile double pr = chunk_range * (double)index_real;
    volatile double pi = chunk_range * (double)index_imag;
    *range = chunk_range;
    *start_r = -2.0 + pr;
    *start_i = -2.0 + pi;
    return MBK_OK;
}

int mbk_view_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                    int32_t *d_counts, uint8_t *d_bytes, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_tile(ctx, view, mrd, flags, d_counts, d_bytes, (hipStream_t)hip_stream);
}

// The window's TileArgs as far as the host-side tests need them (axes + window)
static TileArgs view_window_args(const mbk_view *v)
{
    TileArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    return a;
}

// Does every sample of the window lie outside the circle |c| = 2, with room to spare: |c|^2 >= 4 (1 + m), m = 1e-8
// (fp64) / 1e-4 (fp32)?  The samples of an axis lie between its two end samples up to a few units in the last place
// (k * step + start is monotonic in k before rounding), which the margin covers 10^7 times over.
static bool view_outside_circle2(const mbk_view *v, bool f32)
{
    const TileArgs a = view_window_args(v);
    const double x0 = axis_value_host(a.re, a.col0), x1 = axis_value_host(a.re, a.col0 + a.ncols - 1u);
    const double y0 = axis_value_host(a.im, a.row0), y1 = axis_value_host(a.im, a.row0 + a.nrows - 1u);
    const double xlo = std::fmin(x0, x1), xhi = std::fmax(x0, x1), ylo = std::fmin(y0, y1), yhi = std::fmax(y0, y1);
    const double dx = (xlo <= 0.0 && 0.0 <= xhi) ? 0.0 : std::fmin(std::fabs(xlo), std::fabs(xhi));
    const double dy = (ylo <= 0.0 && 0.0 <= yhi) ? 0.0 : std::fmin(std::fabs(ylo), std::fabs(yhi));
    const double rmin2 = dx * dx + dy * dy;
    return rmin2 >= 4.0 * (1.0 + (f32 ? 1e-4 : 1e-8));
}

static double view_probe_share(mbk_ctx *ctx, const mbk_view *v) { return window_heavy_share(ctx, view_window_args(v)); }

// enqueue kernel + reduction + D2H of one tile on a slot's stream (no host synchronisation)
static int submit_view(mbk_ctx *ctx, Slot &sl, const mbk_view *view, uint32_t mrd, uint32_t flags,
                       int32_t *h_counts, uint8_t *h_bytes)
{
    if (sl.busy) return fail(ctx, MBK_ERR_INVALID, "slot still has a tile in flight: call mbk_wait first");
    const bool wc = (flags & MBK_WANT_COUNTS) != 0, wb = (flags & MBK_WANT_BYTES) != 0;
    if (flags & MBK_DEEP_BLA) return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_BLA is a flag of the deep view calls");
    if (flags & MBK_DEEP_XBLA) return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA is a flag of the extended-range deep view calls");
    int rc = check_wanted(ctx, flags, h_counts, h_bytes);
    if (rc != MBK_OK) return rc;
    bool dummy;
    rc = validate_view(ctx, view, &dummy, (flags & MBK_PRECISION_F32) != 0);
    if (rc != MBK_OK) return rc;
    const size_t px = (size_t)view->ncols * view->nrows;
    const bool lazy = wb && (flags & MBK_LAZY_UNIFORM) != 0;
    const bool f32 = (flags & MBK_PRECISION_F32) != 0;
    sl.immediate = false;
    if (lazy && !wc && mrd >= 256u && mrd <= 0x7fffffffu && view_outside_circle2(view, f32)) {
        // Every pixel of the window has |c| >= 2 (1 + 1e-8): the reference's first update z1 = c^2 + c has
        // |z1| = |c| |c + 1| >= |c| (|c| - 1) > 2, so calc_mb_value returns 1 for each of them (WorkerCUDA.py:54-63; the proof
        // with the rounding errors of the five operations: tests/test_oracle.py::test_outside_circle_escapes_at_step_one)
        // and the quantised byte is ceil(256 / mrd) = 1 for mrd >= 256: DataChunk.cs:87's "Immediate" chunk.  With
        // MBK_LAZY_UNIFORM such a tile is not copied anyway, so nothing is enqueued at all: the corners of [-2, 2]^2 outside
        // the inscribed circle, 1 - pi/4 = 21 % of the tiles of a deep pyramid level (32 of level 16's 256).
        std::memset(&sl.imm, 0, sizeof(sl.imm));
        sl.imm.pixel_iterations = (uint64_t)px;
        sl.imm.all_bytes_one = 1u;
        sl.imm.rle_runs = 1ull;
        sl.immediate = true;
        sl.lazy_h_bytes = nullptr;
        sl.busy = true;
        sl.with_bytes = true;
        if (&sl == &ctx->s[0]) ctx->last_px = 0;   // (no bytes on the device: mbk_serialize_last has nothing to read)
        return MBK_OK;
    }
    rc = ensure_buffers(ctx, sl, px);
    if (rc != MBK_OK) return rc;
    // counts are always produced on the device (they feed the stats reduction); only what the
    // caller asked for crosses PCIe.
    const uint32_t dev_flags = (flags & (MBK_KERNEL_MASK | MBK_PRECISION_F32)) | MBK_WANT_COUNTS | (wb ? MBK_WANT_BYTES : 0u);
    // The statistics: a pass over counts (+ bytes) after the tile kernel -- unless the kernel that serves this window can
    // add up pixel-iterations and never-escaped pixels itself (the finish-in-place light pass: all-exterior tiles, 3 in 4
    // of a pyramid level).  Then no int32 count is written unless the caller asked for counts, and the pass reads the
    // bytes only (all-0 / all-1 flags, run count): 16 MiB instead of 80 for a DataChunk.
    MBK_HIP(ctx, hipMemsetAsync(sl.d_red, 0, sizeof(ReduceSlot) * mbk::kReduceSlots, sl.stream));
    FuseStats fuse = {sl.d_red, !wc, false};
    MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
    rc = launch_tile(ctx, view, mrd, dev_flags, sl.d_counts, sl.d_bytes, sl.stream, nullptr, &fuse);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipEventRecord(sl.ev_k1, sl.stream));
    rc = launch_reduce(ctx, sl, fuse.fused ? nullptr : sl.d_counts, wb ? sl.d_bytes : nullptr, px, mrd, sl.stream, false);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
    // MBK_LAZY_UNIFORM: whether the tile is uniform is known only when its statistics are -- deciding the copy then costs a
    // synchronisation, an enqueue and a second synchronisation per tile (round 4: 20 % of a pyramid level's wall time).  So
    // the copy is enqueued NOW unless the host's 16 x 16 probe of the window says "every pixel gone within 4 steps" (the
    // all-exterior tile: counts 1..4, byte 1 everywhere for mrd >= 1024); a uniform tile that was copied anyway (an all-interior one)
    // wasted 0.3 ms of the copy engine beside its own 2 ms kernel, a non-uniform one that was not takes the old path in
    // mbk_wait.  Either way the caller is told by the stats whether h_bytes matters.
    bool lazy_deferred = false;
    if (lazy) lazy_deferred = view_probe_share(ctx, view) == 0.0;
    if (wb && !lazy_deferred) MBK_HIP(ctx, hipMemcpyAsync(h_bytes, sl.d_bytes, px, hipMemcpyDeviceToHost, sl.stream));
    if (wc) MBK_HIP(ctx, hipMemcpyAsync(h_counts, sl.d_counts, px * sizeof(int32_t), hipMemcpyDeviceToHost, sl.stream));
    MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
    sl.lazy_h_bytes = lazy_deferred ? h_bytes : nullptr;
    sl.lazy_px = px;
    sl.busy = true;
    sl.with_bytes = wb;
    if (&sl == &ctx->s[0]) ctx->last_px = wb ? px : 0;
    return MBK_OK;
}

static int wait_slot(mbk_ctx *ctx, Slot &sl, mbk_stats *stats)
{
    if (!sl.busy) return fail(ctx, MBK_ERR_INVALID, "nothing was submitted on this slot");
    if (sl.immediate) {   // decided on the host at submit: nothing is in flight
        sl.busy = false;
        sl.immediate = false;
        if (stats) *stats = sl.imm;
        return MBK_OK;
    }
    MBK_HIP(ctx, hipStreamSynchronize(sl.stream));
    sl.busy = false;
    if (sl.lazy_h_bytes) {   // MBK_LAZY_UNIFORM: copy the bytes only if the tile is not all-0 / all-1
        uint8_t *dst = sl.lazy_h_bytes;
        sl.lazy_h_bytes = nullptr;
        const ReduceOut t = reduce_total(sl);
        if (t.any_byte_not_zero != 0 && t.any_byte_not_one != 0) {
            MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
            MBK_HIP(ctx, hipMemcpyAsync(dst, sl.d_bytes, sl.lazy_px, hipMemcpyDeviceToHost, sl.stream));
            MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
            MBK_HIP(ctx, hipStreamSynchronize(sl.stream));
        }
    }
    return stats ? slot_stats(ctx, sl, stats, sl.with_bytes) : MBK_OK;
}

static void datachunk_view(mbk_view *v, double sr, double si, double range)
{
    v->start_r = sr;
    v->start_i = si;
    v->range_r = range;
    v->range_i = range;
    v->width = v->height = MBK_CHUNK_DEFINITION;
    v->col0 = v->row0 = 0;
    v->ncols = v->nrows = MBK_CHUNK_DEFINITION;
}

int mbk_view_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                     int32_t *h_counts, uint8_t *h_bytes, mbk_stats *stats)
{
    if (!ctx || !view) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    int rc = submit_view(ctx, ctx->s[0], view, mrd, flags, h_counts, h_bytes);
    if (rc != MBK_OK) return rc;
    return wait_slot(ctx, ctx->s[0], stats);
}

int mbk_datachunk_submit(mbk_ctx *ctx, int slot, uint32_t level, uint32_t mrd, uint32_t index_real,
                         uint32_t index_imag, uint8_t *h_bytes, int32_t *h_counts)
{
    return mbk_datachunk_submit_ex(ctx, slot, level, mrd, index_real, index_imag, h_bytes, h_counts, 0u);
}

int mbk_datachunk_submit_ex(mbk_ctx *ctx, int slot, uint32_t level, uint32_t mrd, uint32_t index_real,
                            uint32_t index_imag, uint8_t *h_bytes, int32_t *h_counts, uint32_t flags)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (slot < 0 || slot >= MBK_SLOTS) return fail(ctx, MBK_ERR_INVALID, "slot out of range");
    if (!h_bytes) return fail(ctx, MBK_ERR_INVALID, "h_bytes is NULL");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    double sr, si, range;
    int rc = mbk_datachunk_geometry(level, index_real, index_imag, &sr, &si, &range);
    if (rc != MBK_OK) {
        ctx->err = g_err;
        return rc;
    }
    mbk_view v;
    datachunk_view(&v, sr, si, range);
    return submit_view(ctx, ctx->s[slot], &v, mrd,
                       MBK_WANT_BYTES | (h_counts ? MBK_WANT_COUNTS : 0u) | (flags & (MBK_LAZY_UNIFORM | MBK_KERNEL_MASK)),
                       h_counts, h_bytes);
}

int mbk_view_submit(mbk_ctx *ctx, int slot, const mbk_view *view, uint32_t mrd, uint32_t flags,
                    int32_t *h_counts, uint8_t *h_bytes)
{
    if (!ctx || !view) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    if (slot < 0 || slot >= MBK_SLOTS) return fail(ctx, MBK_ERR_INVALID, "slot out of range");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    return submit_view(ctx, ctx->s[slot], view, mrd, flags, h_counts, h_bytes);
}

int mbk_view_needs_literal_doubling(const mbk_view *view, uint32_t flags, int *literal)
{
    if (!view || !literal) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    const int rc = validate_view(nullptr, view, &safe, (flags & MBK_PRECISION_F32) != 0);
    if (rc != MBK_OK) return rc;
    *literal = safe ? 1 : 0;
    return MBK_OK;
}

int mbk_view_outside_circle(const mbk_view *view, uint32_t flags, int *outside)
{
    if (!view || !outside) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    bool dummy;
    const bool f32 = (flags & MBK_PRECISION_F32) != 0;
    const int rc = validate_view(nullptr, view, &dummy, f32);
    if (rc != MBK_OK) return rc;
    *outside = view_outside_circle2(view, f32) ? 1 : 0;
    return MBK_OK;
}

int mbk_wait(mbk_ctx *ctx, int slot, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (slot < 0 || slot >= MBK_SLOTS) return fail(ctx, MBK_ERR_INVALID, "slot out of range");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    return wait_slot(ctx, ctx->s[slot], stats);
}

int mbk_datachunk(mbk_ctx *ctx, uint32_t level, uint32_t mrd, uint32_t index_real,
                  uint32_t index_imag, uint8_t *h_bytes, int32_t *h_counts, mbk_stats *stats)
{
    int rc = mbk_datachunk_submit(ctx, 0, level, mrd, index_real, index_imag, h_bytes, h_counts);
    if (rc != MBK_OK) return rc;
    return wait_slot(ctx, ctx->s[0], stats);
}

int mbk_view_launch_smooth(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                           int32_t *d_counts, double *d_smooth, void *hip_stream)
{
    if (!ctx || !d_smooth) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t f = (flags & (MBK_KERNEL_MASK | MBK_PRECISION_F32 | MBK_DEEP_XBLA)) | (d_counts ? MBK_WANT_COUNTS : 0u);
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_tile(ctx, view, mrd, f, d_counts, nullptr, (hipStream_t)hip_stream, d_smooth);
}

int mbk_view_compute_smooth(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                            int32_t *h_counts, double *h_smooth, mbk_stats *stats)
{
    if (!ctx || !view || !h_smooth) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    int rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    bool dummy;
    rc = validate_view(ctx, view, &dummy);
    if (rc != MBK_OK) return rc;
    return compute_values(ctx, (size_t)view->ncols * view->nrows, mrd, h_counts, h_smooth, stats,
                          [&](int32_t *d_counts, double *d_smooth, hipStream_t stream) {
                              return launch_tile(ctx, view, mrd, (flags & (MBK_KERNEL_MASK | MBK_DEEP_XBLA)) | MBK_WANT_COUNTS, d_counts, nullptr, stream, d_smooth);
                          });
}

// ---- distance estimates (mbk_distance.h; mbk.h "Distance estimates") ---------------------------------------------------

// Everything a distance launch can refuse, before anything is allocated, enqueued or written.
static int distance_check(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, bool *safe)
{
    int rc = validate_view(ctx, view, safe);
    if (rc != MBK_OK) return rc;
    if (mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    if (flags & MBK_DEEP_XBLA) return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA is a flag of the extended-range deep view calls");
    if (flags & MBK_PRECISION_F32) return fail(ctx, MBK_ERR_INVALID, "distance estimates are implemented in binary64 only");
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if (kernel > MBK_KERNEL_SCAN) return fail(ctx, MBK_ERR_INVALID, "unknown MBK_KERNEL_* selector");
    if (kernel == MBK_KERNEL_SIMPLE || kernel == MBK_KERNEL_REFILL)
        return fail(ctx, MBK_ERR_INVALID, "distance estimates are implemented with the scan / asm / group kernels only");
    return MBK_OK;
}

// A checked launch.  Kernel "asm": one pass, the derivative rides in a per-step escape loop.  Every other selector: the
// escape kernels it names write the counts, then the derivative pass runs each escaped pixel for exactly its count.
static int launch_distance(mbk_ctx *ctx, const mbk_view *v, uint32_t mrd, uint32_t flags, bool safe, int32_t *d_counts,
                           double *d_distance, hipStream_t stream)
{
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    const bool one_pass = kernel == MBK_KERNEL_ASM;
    if (!one_pass) {
        int rc = launch_count_pass(ctx, (size_t)v->ncols * v->nrows, stream, &d_counts, [&](int32_t *counts) {
            return launch_tile(ctx, v, mrd, kernel | MBK_WANT_COUNTS, counts, nullptr, stream);
        });
        if (rc != MBK_OK) return rc;
    }
    mbk::DistanceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.mrd = (int32_t)mrd;
    a.counts_in = one_pass ? nullptr : d_counts;
    a.counts_out = one_pass ? d_counts : nullptr;
    a.distance = d_distance;
    const dim3 grid(a.blocks_x * ((v->nrows + 7u) / 8u)), block(64);   // (at most 2^31 / 64 blocks: validate_view)
    if (one_pass) {
        if (safe) hipLaunchKernelGGL((mbk::distance_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mbk::distance_kernel<true, true>), grid, block, 0, stream, a);
    } else {
        if (safe) hipLaunchKernelGGL((mbk::distance_kernel<false, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mbk::distance_kernel<true, false>), grid, block, 0, stream, a);
    }
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

double mbk_distance_value_host(double mag, double dmag, int32_t count)
{
    return mbk::distance_value(mag, dmag, count);
}

// ---- normals for relief shading (mbk_relief.h; mbk.h "Relief shading") -------------------------------------------------

// Everything a normal launch can refuse, before anything is allocated, enqueued or written: what a distance launch refuses,
// and every flag that is no kernel selector.
static int normal_check(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, bool *safe)
{
    int rc = distance_check(ctx, view, mrd, flags, safe);
    if (rc != MBK_OK) return rc;
    if (flags & ~(uint32_t)MBK_KERNEL_MASK) return fail(ctx, MBK_ERR_INVALID, "normals take kernel selection only (binary64, no other flag)");
    return MBK_OK;
}

// The relief kernel on a checked view.  d_counts_in: the two-pass form on these counts; NULL: the one-pass form, which writes
// its counts to d_counts_out where that is given.  d_distance may be null.
static int launch_relief_kernel(mbk_ctx *ctx, const mbk_view *v, uint32_t mrd, bool safe, const int32_t *d_counts_in,
                                int32_t *d_counts_out, double *d_normal, double *d_distance, hipStream_t stream)
{
    const bool one_pass = d_counts_in == nullptr;
    mbk::ReliefArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.mrd = (int32_t)mrd;
    a.counts_in = d_counts_in;
    a.counts_out = one_pass ? d_counts_out : nullptr;
    a.normal = d_normal;
    a.distance = d_distance;
    const dim3 grid(a.blocks_x * ((v->nrows + 7u) / 8u)), block(64);   // (at most 2^31 / 64 blocks: validate_view)
    if (one_pass) {
        if (safe) hipLaunchKernelGGL((mbk::relief_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mbk::relief_kernel<true, true>), grid, block, 0, stream, a);
    } else {
        if (safe) hipLaunchKernelGGL((mbk::relief_kernel<false, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mbk::relief_kernel<true, false>), grid, block, 0, stream, a);
    }
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// A checked launch, in the two forms of launch_distance: kernel "asm" in one pass; every other selector has the escape kernels
// it names write the counts (into the stream's scratch when the caller wants none) and runs the two-pass form on them.
static int launch_normal(mbk_ctx *ctx, const mbk_view *v, uint32_t mrd, uint32_t flags, bool safe, int32_t *d_counts,
                         double *d_normal, double *d_distance, hipStream_t stream)
{
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if (kernel == MBK_KERNEL_ASM) return launch_relief_kernel(ctx, v, mrd, safe, nullptr, d_counts, d_normal, d_distance, stream);
    int rc = launch_count_pass(ctx, (size_t)v->ncols * v->nrows, stream, &d_counts, [&](int32_t *counts) {
        return launch_tile(ctx, v, mrd, kernel | MBK_WANT_COUNTS, counts, nullptr, stream);
    });
    if (rc != MBK_OK) return rc;
    return launch_relief_kernel(ctx, v, mrd, safe, d_counts, nullptr, d_normal, d_distance, stream);
}

int mbk_view_launch_normal(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *d_counts, double *d_normal,
                           double *d_distance, void *hip_stream)
{
    if (!ctx || !d_normal) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    int rc = normal_check(ctx, view, mrd, flags, &safe);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_normal & 7u) return fail(ctx, MBK_ERR_INVALID, "d_normal must be 8-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_normal(ctx, view, mrd, flags, safe, d_counts, d_normal, d_distance, (hipStream_t)hip_stream);
}

int mbk_view_compute_normal(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *h_counts, double *h_normal,
                            double *h_distance, mbk_stats *stats)
{
    if (!ctx || !view || !h_normal) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    int rc = normal_check(ctx, view, mrd, flags, &safe);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    const size_t px = (size_t)view->ncols * view->nrows;
    return compute_values(ctx, px, mrd, h_counts, h_normal, stats,
                          [&](int32_t *d_counts, double *d_normal, hipStream_t stream) {
                              return launch_normal(ctx, view, mrd, flags, safe, d_counts, d_normal, h_distance ? d_normal + 2u * px : nullptr, stream);
                          },
                          false, nullptr, 2u, h_distance);
}

int mbk_normal_value_host(double zr, double zi, double dr, double di, int32_t count, double out[2])
{
    if (!out) return fail(nullptr, MBK_ERR_INVALID, "out is NULL");
    mbk::normal_value(zr, zi, dr, di, count, out);
    return MBK_OK;
}

uint32_t mbk_relief_shade_host(double nx, double ny, double lx, double ly, double h)
{
    return mbk::relief_shade(nx, ny, lx, ly, h);
}

// ---- stripe averages (mbk_stripe.h; mbk.h "Stripe-average colouring") --------------------------------------------------

// Everything a stripe launch can refuse, before anything is allocated, enqueued or written: what a distance launch refuses,
// kernel "asm" (there is no one-pass form), every flag that is no kernel selector, and a density out of range.
static int stripe_check(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t density, uint32_t skip, bool *safe)
{
    int rc = distance_check(ctx, view, mrd, flags, safe);
    if (rc != MBK_OK) return rc;
    if (flags & ~(uint32_t)MBK_KERNEL_MASK) return fail(ctx, MBK_ERR_INVALID, "stripe averages take kernel selection only (binary64, no other flag)");
    if ((flags & MBK_KERNEL_MASK) == MBK_KERNEL_ASM) return fail(ctx, MBK_ERR_INVALID, "stripe averages have no one-pass form: take the default selector, scan or group");
    if (density < 1u || density > mbk::kStripeDensityMax) return fail(ctx, MBK_ERR_INVALID, "density must lie in 1 .. 16");
    if (skip > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "skip must lie in 0 .. 2^31 - 1");
    return MBK_OK;
}

// The stripe kernel on a checked view and the counts of its pixels.  d_state may be null.
static int launch_stripe_kernel(mbk_ctx *ctx, const mbk_view *v, bool safe, uint32_t density, uint32_t skip, const int32_t *d_counts,
                                double *d_stripe, double *d_state, hipStream_t stream)
{
    mbk::StripeArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.density = density;
    a.skip = skip;
    a.counts_in = d_counts;
    a.value = d_stripe;
    a.state = d_state;
    a.px = (uint64_t)v->ncols * v->nrows;
    const dim3 grid(a.blocks_x * ((v->nrows + 7u) / 8u)), block(64);   // (at most 2^31 / 64 blocks: validate_view)
    if (safe) hipLaunchKernelGGL(mbk::stripe_kernel<false>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(mbk::stripe_kernel<true>, grid, block, 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// A checked launch: the escape kernels the selector names write the counts (into the stream's scratch when the caller wants
// none), then the stripe kernel replays each escaped pixel for exactly its count.
static int launch_stripe(mbk_ctx *ctx, const mbk_view *v, uint32_t mrd, uint32_t flags, bool safe, uint32_t density, uint32_t skip,
                         int32_t *d_counts, double *d_stripe, double *d_state, hipStream_t stream)
{
    int rc = launch_count_pass(ctx, (size_t)v->ncols * v->nrows, stream, &d_counts, [&](int32_t *counts) {
        return launch_tile(ctx, v, mrd, (flags & MBK_KERNEL_MASK) | MBK_WANT_COUNTS, counts, nullptr, stream);
    });
    if (rc != MBK_OK) return rc;
    return launch_stripe_kernel(ctx, v, safe, density, skip, d_counts, d_stripe, d_state, stream);
}

int mbk_view_launch_stripe(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t density, uint32_t skip,
                           int32_t *d_counts, double *d_stripe, void *d_state, void *hip_stream)
{
    if (!ctx || !d_stripe) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    int rc = stripe_check(ctx, view, mrd, flags, density, skip, &safe);
    if (rc != MBK_OK) return rc;
    if (((uintptr_t)d_stripe | (uintptr_t)d_state) & 7u) return fail(ctx, MBK_ERR_INVALID, "d_stripe and d_state must be 8-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_stripe(ctx, view, mrd, flags, safe, density, skip, d_counts, d_stripe, (double *)d_state, (hipStream_t)hip_stream);
}

int mbk_view_compute_stripe(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t density, uint32_t skip,
                            int32_t *h_counts, double *h_stripe, void *h_state, mbk_stats *stats)
{
    if (!ctx || !view || !h_stripe) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    int rc = stripe_check(ctx, view, mrd, flags, density, skip, &safe);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    const size_t px = (size_t)view->ncols * view->nrows;
    return compute_values(ctx, px, mrd, h_counts, h_stripe, stats,
                          [&](int32_t *d_counts, double *d_stripe, hipStream_t stream) {
                              return launch_stripe(ctx, view, mrd, flags, safe, density, skip, d_counts, d_stripe, h_state ? d_stripe + px : nullptr, stream);
                          },
                          false, nullptr, 1u, (double *)h_state, nullptr, 4u);
}

int mbk_stripe_state_host(double c_r, double c_i, uint32_t mrd, uint32_t density, uint32_t skip, mbk_stripe_state *out)
{
    if (!out) return fail(nullptr, MBK_ERR_INVALID, "out is NULL");
    if (mrd > 0x7fffffffu) return fail(nullptr, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    if (density < 1u || density > mbk::kStripeDensityMax) return fail(nullptr, MBK_ERR_INVALID, "density must lie in 1 .. 16");
    if (skip > 0x7fffffffu) return fail(nullptr, MBK_ERR_INVALID, "skip must lie in 0 .. 2^31 - 1");
    // the literal doubling throughout: the contract's step, which the fused form equals wherever a launch takes it
    double m = 0.0;
    std::memset(out, 0, sizeof(*out));
    out->n = mbk::julia_count<false>(c_r, c_i, c_r, c_i, (int32_t)mrd, &m);
    if (out->n > 0) {
        const mbk::StripeState st = mbk::stripe_replay<false>(c_r, c_i, out->n, density, skip);
        out->N = st.N;
        out->cnt = st.cnt;
        out->S = st.S;
        out->t_last = st.t_last;
        out->mag = st.mag;
    }
    out->v = mbk::stripe_value(out->S, out->t_last, out->cnt, out->mag, out->n);
    return MBK_OK;
}

double mbk_stripe_value_host(double S, double t_last, int32_t cnt, double mag, int32_t count)
{
    return mbk::stripe_value(S, t_last, cnt, mag, count);
}

uint32_t mbk_stripe_shade_host(double v, double lo, double gain)
{
    return mbk::stripe_shade(v, lo, gain);
}

// ---- interior views (mbk_interior.h; mbk.h "Interior views") -----------------------------------------------------------

// Everything an interior launch can refuse, before anything is allocated, enqueued or written.
static int interior_check(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, bool *safe)
{
    int rc = validate_view(ctx, view, safe);
    if (rc != MBK_OK) return rc;
    if (mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    if (flags & ~(uint32_t)MBK_KERNEL_MASK) return fail(ctx, MBK_ERR_INVALID, "interior views take kernel selection only (binary64, no other flag)");
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if (kernel != MBK_KERNEL_DEFAULT && kernel != MBK_KERNEL_SCAN && kernel != MBK_KERNEL_GROUP)
        return fail(ctx, MBK_ERR_INVALID, "interior views are implemented with the default / scan / group kernels only");
    return MBK_OK;
}

// A checked launch: the escape kernels the selector names write the counts, then the interior pass runs every count-0 pixel.
// d_period or d_distance may be null.
static int launch_interior(mbk_ctx *ctx, const mbk_view *v, uint32_t mrd, uint32_t flags, bool safe, int32_t *d_counts,
                           int32_t *d_period, double *d_distance, hipStream_t stream)
{
    int rc = launch_count_pass(ctx, (size_t)v->ncols * v->nrows, stream, &d_counts, [&](int32_t *counts) {
        return launch_tile(ctx, v, mrd, (flags & MBK_KERNEL_MASK) | MBK_WANT_COUNTS, counts, nullptr, stream);
    });
    if (rc != MBK_OK) return rc;
    mbk::InteriorArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.mrd = (int32_t)mrd;
    a.counts_in = d_counts;
    a.period = d_period;
    a.distance = d_distance;
    const dim3 grid(a.blocks_x * ((v->nrows + 7u) / 8u)), block(64);   // (at most 2^31 / 64 blocks: validate_view)
    if (safe) hipLaunchKernelGGL(mbk::interior_kernel<false>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(mbk::interior_kernel<true>, grid, block, 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

int mbk_view_interior_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *d_counts,
                             int32_t *d_period, double *d_distance, void *hip_stream)
{
    if (!ctx || (!d_period && !d_distance)) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    int rc = interior_check(ctx, view, mrd, flags, &safe);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_interior(ctx, view, mrd, flags, safe, d_counts, d_period, d_distance, (hipStream_t)hip_stream);
}

int mbk_view_interior_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *h_counts,
                              int32_t *h_period, double *h_distance, mbk_stats *stats)
{
    if (!ctx || !view || (!h_period && !h_distance)) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    int rc = interior_check(ctx, view, mrd, flags, &safe);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    const size_t px = (size_t)view->ncols * view->nrows;
    return compute_values(ctx, px, mrd, h_counts, h_distance, stats,
                          [&](int32_t *d_counts, double *d_distance, hipStream_t stream) {
                              return launch_interior(ctx, view, mrd, flags, safe, d_counts, h_period ? (int32_t *)(d_distance + px) : nullptr,
                                                     h_distance ? d_distance : nullptr, stream);
                          },
                          true, h_period);
}

int mbk_interior_host(double c_r, double c_i, uint32_t mrd, int32_t *count, int32_t *period, int32_t *cycle_len, double *de)
{
    if (!count) return fail(nullptr, MBK_ERR_INVALID, "count is NULL");
    if (mrd > 0x7fffffffu) return fail(nullptr, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    // the literal doubling throughout: the contract's step, which the fused form equals wherever a launch takes it
    double mag = 0.0, d = 0.0;
    int32_t L = 0, p = 0;
    *count = mbk::julia_count<false>(c_r, c_i, c_r, c_i, (int32_t)mrd, &mag);
    mbk::interior_pixel<false>(c_r, c_i, (int32_t)mrd, *count, L, p, d);
    if (period) *period = p;
    if (cycle_len) *cycle_len = L;
    if (de) *de = d;
    return MBK_OK;
}

int mbk_serialize_last(mbk_ctx *ctx, uint8_t *h_out, uint64_t cap, uint64_t *size, uint32_t *codec)
{
    if (!ctx || !h_out || !size || !codec) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    int rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    const size_t n = ctx->last_px;
    if (n == 0) return fail(ctx, MBK_ERR_INVALID, "no tile with quantised bytes has been computed on this ctx");
    const uint32_t nblocks = (uint32_t)((n + mbk::kRleBlock - 1) / mbk::kRleBlock);
    // scratch layout (all 256-byte aligned): block counts | total | run_start | run_value | out
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // RLE is only emitted when 1 + 5*runs < 1 + n, i.e. for at most n/5 runs and n output bytes
    const size_t max_runs = n / 5 + 1;
    const size_t off_cnt = 0, off_tot = align(off_cnt + (size_t)nblocks * 4), off_start = align(off_tot + 8),
                 off_val = align(off_start + max_runs * 4), off_out = align(off_val + max_runs),
                 total_bytes = off_out + 1 + n;
    rc = grow(ctx, ctx->d_rle, ctx->rle_cap_px, n, total_bytes);
    if (rc != MBK_OK) return rc;
    uint32_t *d_cnt = (uint32_t *)(ctx->d_rle + off_cnt);
    unsigned long long *d_tot = (unsigned long long *)(ctx->d_rle + off_tot);
    uint32_t *d_start = (uint32_t *)(ctx->d_rle + off_start);
    uint8_t *d_val = ctx->d_rle + off_val, *d_out = ctx->d_rle + off_out;
    hipStream_t s = ctx->s[0].stream;
    hipLaunchKernelGGL(mbk::rle_count_kernel, dim3(nblocks), dim3(mbk::kRleBlock), 0, s, ctx->s[0].d_bytes, (uint64_t)n, d_cnt);
    hipLaunchKernelGGL(mbk::rle_scan_kernel, dim3(1), dim3(1024), 0, s, d_cnt, nblocks, d_tot);
    MBK_HIP(ctx, hipGetLastError());
    unsigned long long runs = 0;
    MBK_HIP(ctx, hipMemcpyAsync(&runs, d_tot, sizeof(runs), hipMemcpyDeviceToHost, s));
    MBK_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t raw_size = 1 + (uint64_t)n, rle_size = 1 + 5 * (uint64_t)runs;
    // DataChunk.Serialize keeps the first serializer (Raw) unless a later one is strictly smaller
    const bool use_rle = rle_size < raw_size;
    *codec = use_rle ? MBK_CODEC_RLE : MBK_CODEC_RAW;
    *size = use_rle ? rle_size : raw_size;
    if (cap < *size) return fail(ctx, MBK_ERR_INVALID, "output buffer too small for the serialised chunk");
    if (use_rle) {
        hipLaunchKernelGGL(mbk::rle_scatter_kernel, dim3(nblocks), dim3(mbk::kRleBlock), 0, s, ctx->s[0].d_bytes,
                           (uint64_t)n, d_cnt, d_start, d_val);
        hipLaunchKernelGGL(mbk::rle_emit_kernel, dim3((uint32_t)((runs + 255) / 256)), dim3(256), 0, s, d_start,
                           d_val, (uint64_t)runs, (uint64_t)n, d_out);
        MBK_HIP(ctx, hipGetLastError());
        MBK_HIP(ctx, hipMemcpyAsync(h_out, d_out, rle_size, hipMemcpyDeviceToHost, s));
    } else {
        h_out[0] = MBK_CODEC_RAW;
        MBK_HIP(ctx, hipMemcpyAsync(h_out + 1, ctx->s[0].d_bytes, n, hipMemcpyDeviceToHost, s));
    }
    MBK_HIP(ctx, hipStreamSynchronize(s));
    return MBK_OK;
}

int mbk_set_option(mbk_ctx *ctx, int option, uint32_t value)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    bool ok = false;
    switch (option) {
        case MBK_OPT_ORDER: ok = value <= 3u; break;
        case MBK_OPT_WAVES_PER_WG: ok = value == 1u || value == 2u || value == 4u; break;
        case MBK_OPT_GROUP_STEPS: ok = value == 4u || value == 8u || value == 16u || value == 32u; break;
        case MBK_OPT_EXACT_STEPS: ok = value <= 4096u; break;
        case MBK_OPT_PROBE_STEPS: ok = value >= 2u && value <= 65536u; break;
        case MBK_OPT_SCAN_WAVES: ok = value >= 1u && value <= 8u; break;
        case MBK_OPT_SCAN_XCD_MAP: ok = value <= 1u; break;
        case MBK_OPT_SCAN_COL_PERIOD: ok = value <= 65536u; break;
        case MBK_OPT_HEAVY_SHARE: ok = value <= 65536u; break;
        case MBK_OPT_RF_LIVEMIN: ok = value <= 63u; break;
        case MBK_OPT_RF_PATIENCE: ok = value >= 16u && value <= (1u << 20); break;
        case MBK_OPT_RF_BATCH: ok = value >= 1u && value <= 64u; break;
        case MBK_OPT_RF_WAVES: ok = value >= 1u && value <= 8u; break;
        case MBK_OPT_CYCLE_DETECT: ok = value <= 1u; break;
        case MBK_OPT_PROBE_MID: ok = value >= 2u && value <= 65537u; break;
        case MBK_OPT_PREPASS_OVERLAP: ok = value <= 2u; break;
        case MBK_OPT_CLASSIFY_WG: ok = value >= 64u && value <= 1024u && value % 64u == 0u; break;
        case MBK_OPT_SCAN_STRIP: ok = value <= 1u; break;
        case MBK_OPT_CYCLE_WINDOW: ok = value <= 65536u; break;
        case MBK_OPT_EXACT_LONG: ok = value <= 4096u; break;
        case MBK_OPT_SCAN_INLINE: ok = value <= 1u; break;
        case MBK_OPT_WAVE_LIMIT: ok = value <= 7u; break;
        case MBK_OPT_UNITS_MIN_LIGHT: ok = value <= 65536u; break;
        case MBK_OPT_XCD_BALANCE: ok = value <= 2u; break;
        case MBK_OPT_M_LATE: ok = value <= 65536u; break;
        case MBK_OPT_H_SETTLED: ok = value <= 30u; break;
        case MBK_OPT_SPILL_FIRST: ok = value <= 65536u && value % 32u == 0u; break;
        case MBK_OPT_SPILL_LANES: ok = value >= 1u && value <= 32u; break;
        case MBK_OPT_SPILL_MIN_MRD: ok = true; break;
        case MBK_OPT_SPILL_MIN_BLOCKS: ok = value <= 31u; break;
        case MBK_OPT_SPILL_CYC_SHIFT: ok = value <= 31u; break;
        case MBK_OPT_SURE_INTERIOR: ok = value <= 2u; break;
        default: return fail(ctx, MBK_ERR_INVALID, "unknown MBK_OPT_* selector");
    }
    if (!ok) return fail(ctx, MBK_ERR_INVALID, "option value out of range");
    ctx->opt[option] = value;
    return MBK_OK;
}

int mbk_get_option(mbk_ctx *ctx, int option, uint32_t *value)
{
    if (!ctx || !value) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    if (option >= MBK_INFO_SCAN_WG_PER_CU && option < MBK_INFO_SCAN_WG_PER_CU + 4) {
        const int k = option - MBK_INFO_SCAN_WG_PER_CU;   // [f64 scan, f64 heavy, f32 scan, f32 heavy]
        *value = (uint32_t)ctx->scan_occ[k >> 1][k & 1];
        return MBK_OK;
    }
    if (option >= MBK_INFO_XCD_SHARE && option < MBK_INFO_XCD_SHARE + 10) {
        // the stream whose units launches have left the most time stamps so far
        const StreamScratch *best = nullptr;
        for (const StreamScratch &sc : ctx->scratch)
            if (!best || sc.xcd_consumed > best->xcd_consumed) best = &sc;
        const int k = option - MBK_INFO_XCD_SHARE;
        *value = !best ? 0u : k < 8 ? (uint32_t)std::lround(best->xcd_f[k] * 1048576.0) : k == 8 ? best->xcd_consumed : best->xcd_issued;
        return MBK_OK;
    }
    if (option == MBK_INFO_SPILL || option == MBK_INFO_SPILL + 1) {
        *value = ctx->spill_launches;
        if (option == MBK_INFO_SPILL) {   // lanes the last such launch handed to its second pass (waits for that launch)
            *value = 0u;
            for (const StreamScratch &sc : ctx->scratch)
                if (sc.stream == ctx->last_spill_stream && sc.spill.d_total && ctx->spill_launches) {
                    unsigned long long t = 0;
                    MBK_HIP(ctx, hipSetDevice(ctx->device));
                    MBK_HIP(ctx, hipStreamSynchronize(sc.stream));
                    MBK_HIP(ctx, hipMemcpy(&t, sc.spill.d_total, sizeof(t), hipMemcpyDeviceToHost));
                    *value = (uint32_t)std::min<unsigned long long>(t, 0xffffffffull);
                }
        }
        return MBK_OK;
    }
    if (option < 0 || option >= MBK_OPT_COUNT_) return fail(ctx, MBK_ERR_INVALID, "unknown MBK_OPT_* selector");
    *value = ctx->opt[option];
    return MBK_OK;
}

// The share arithmetic of the units kernel on the host (no device, no context): the very functions classify_units_kernel and
// tile_units_kernel call, for the CPU tests.
static void shares_from_fractions(const double *f, uint32_t *cum)
{
    double c = 0.0;
    for (uint32_t x = 0; x < 8u; ++x) {
        c += f[x];
        cum[x] = x == 7u ? (1u << 24) : (uint32_t)std::lround(std::min(1.0, std::max(0.0, c)) * (double)(1u << 24));
    }
}

int mbk_units_plan(uint32_t n_h, uint32_t n_v, uint32_t n_m, const double *fractions, uint32_t *plan)
{
    if (!fractions || !plan) return MBK_ERR_INVALID;
    if ((uint64_t)n_h + n_v + n_m > 0x7fffffffull) return MBK_ERR_INVALID;
    uint32_t cum[8];
    shares_from_fractions(fractions, cum);
    mbk::units_plan(n_h, n_v, n_m, cum, 0u, plan, 0u, 0u);
    return MBK_OK;
}

int mbk_units_lookup(const uint32_t *plan, uint32_t id, uint32_t *list, uint32_t *index)
{
    if (!plan || !list || !index) return MBK_ERR_INVALID;
    const uint32_t x = id & 7u;
    bool is_h = false;
    uint32_t i = 0;
    *list = 0u;
    *index = 0u;
    if (id >= plan[2] || !mbk::units_lookup(id, plan[3], plan[4], plan[8u + x], plan[16u + x], plan[24u + x], plan[32u + x], is_h, i))
        return MBK_OK;
    *list = is_h ? 1u : (i < plan[1] ? 2u : 3u);
    *index = is_h ? i : (i < plan[1] ? i : i - plan[1]);
    return MBK_OK;
}

// MBK_OPT_SURE_INTERIOR on the host (no device, no context): the certificate block_pixel evaluates, the blocks of a window that
// pass it whole, and the word a launch would carry.
int mbk_sure_interior_point(double cr, double ci) { return mbk::sure_interior_point(cr, ci) ? 1 : 0; }

int mbk_sure_interior_blocks(const mbk_view *view, uint64_t *certified)
{
    if (!view || !certified) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    bool safe = false;
    const int rc = validate_view(nullptr, view, &safe);
    if (rc != MBK_OK) return rc;
    TileArgs a = view_window_args(view);
    set_window_facts(a, false);
    // the blocks block_pixel calls `interior`: their coordinates are the regular formula's, as evaluated there
    uint64_t n = 0;
    for (uint32_t by = 0; by < a.fast_by_end; ++by)
        for (uint32_t bx = 0; bx < a.fast_bx_end; ++bx) {
            bool all = true;
            for (uint32_t ly = 0; ly < 8u && all; ++ly) {
                const double ci = (double)(a.row0 + by * 8u + ly) * a.im.step + a.im.start;
                for (uint32_t lx = 0; lx < 8u && all; ++lx)
                    all = mbk::sure_interior_point((double)(a.col0 + bx * 8u + lx) * a.re.step + a.re.start, ci);
            }
            n += all ? 1u : 0u;
        }
    *certified = n;
    return MBK_OK;
}

int mbk_sure_interior_flag(const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t cycle_detect, uint32_t option, uint32_t *flag)
{
    if (!view || !flag) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    if (option > 2u || mrd > 0x7fffffffu) return fail(nullptr, MBK_ERR_INVALID, "option value out of range");
    const bool f32 = (flags & MBK_PRECISION_F32) != 0;
    bool safe = false;
    const int rc = validate_view(nullptr, view, &safe, f32);
    if (rc != MBK_OK) return rc;
    TileArgs a = view_window_args(view);
    a.mrd = (int32_t)mrd;
    set_window_facts(a, f32, cycle_detect != 0u, option);
    *flag = a.sure_interior;
    return MBK_OK;
}

int mbk_quantise_counts(mbk_ctx *ctx, const int32_t *h_counts, uint64_t n, uint32_t mrd, uint8_t *h_bytes)
{
    if (!ctx || !h_counts || !h_bytes) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    if (mrd == 0 || mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must be in [1, 2^31)");
    if (n == 0) return MBK_OK;
    if (n > (1ull << 31)) return fail(ctx, MBK_ERR_INVALID, "more than 2^31 counts");
    int rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    rc = ensure_buffers(ctx, sl, (size_t)n);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipMemcpyAsync(sl.d_counts, h_counts, n * sizeof(int32_t), hipMemcpyHostToDevice, sl.stream));
    hipLaunchKernelGGL(mbk::quantise_kernel, dim3(2048), dim3(256), 0, sl.stream, sl.d_counts, sl.d_bytes, n,
                       (int32_t)mrd, mrd >= (1u << 23) ? 1u : 0u, 1.0 / (double)mrd);
    MBK_HIP(ctx, hipGetLastError());
    MBK_HIP(ctx, hipMemcpyAsync(h_bytes, sl.d_bytes, n, hipMemcpyDeviceToHost, sl.stream));
    MBK_HIP(ctx, hipStreamSynchronize(sl.stream));
    ctx->last_px = 0;
    return MBK_OK;
}

int mbk_reduce_counts(mbk_ctx *ctx, const int32_t *d_counts, uint64_t n, uint32_t mrd,
                      void *hip_stream, mbk_stats *stats)
{
    if (!ctx || !d_counts || !stats) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (stream_capturing(s)) return refuse_capture(ctx, "mbk_reduce_counts waits for its result and cannot be captured");
    // partial results live in the STREAM's scratch (not in slot 0's: a tile in flight on slot 0 reduces into those)
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, s, &sc);
    if (rc != MBK_OK) return rc;
    if (!sc->d_red) {
        MBK_HIP(ctx, hipMalloc((void **)&sc->d_red, sizeof(ReduceSlot) * mbk::kReduceSlots));
        MBK_HIP(ctx, hipHostMalloc((void **)&sc->h_red, sizeof(ReduceSlot) * mbk::kReduceSlots, hipHostMallocDefault));
    }
    rc = launch_reduce(ctx, sc->d_red, sc->h_red, d_counts, nullptr, n, mrd, s);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipStreamSynchronize(s));
    std::memset(stats, 0, sizeof(*stats));
    fill_stats_from_reduce(sc->h_red, stats, false);
    return MBK_OK;
}

// ---- deep-zoom views (mbk_deep_orbit.h, mbk_deep.h) ---------------------------------------------------------

int mbk_deep_orbit_create(const char *center_r, const char *center_i, uint32_t precision_bits, uint32_t mrd,
                          mbk_deep_orbit **out)
{
    if (!out) return fail(nullptr, MBK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    mbk_deep_orbit *o = new (std::nothrow) mbk_deep_orbit();
    if (!o) return fail(nullptr, MBK_ERR_NOMEM, "out of host memory");
    std::string why;
    bool ok = false;
    try {
        ok = mbk::build_deep_orbit(center_r, center_i, precision_bits, mrd, &o->o, &why);
    } catch (const std::bad_alloc &) {
        delete o;
        return fail(nullptr, MBK_ERR_NOMEM, "out of host memory for the reference orbit");
    }
    if (!ok) {
        delete o;
        return fail(nullptr, MBK_ERR_INVALID, why);
    }
    *out = o;
    return MBK_OK;
}

void mbk_deep_orbit_destroy(mbk_deep_orbit *orbit) { delete orbit; }

int mbk_deep_orbit_info(const mbk_deep_orbit *orbit, uint32_t *length, uint32_t *escaped, uint32_t *precision_bits,
                        uint32_t *mrd)
{
    if (!orbit) return fail(nullptr, MBK_ERR_INVALID, "orbit is NULL");
    if (length) *length = orbit->o.length;
    if (escaped) *escaped = orbit->o.escaped;
    if (precision_bits) *precision_bits = orbit->o.precision_bits;
    if (mrd) *mrd = orbit->o.mrd;
    return MBK_OK;
}

int mbk_deep_orbit_read(const mbk_deep_orbit *orbit, double *zr, double *zi, uint64_t n)
{
    if (!orbit || !zr || !zi) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    const uint64_t entries = (uint64_t)orbit->o.length + 1u;
    if (n < entries) return fail(nullptr, MBK_ERR_INVALID, "the output holds fewer than length + 1 entries");
    for (uint64_t k = 0; k < entries; ++k) {
        zr[k] = orbit->o.table[4 * k];
        zi[k] = orbit->o.table[4 * k + 1];
    }
    return MBK_OK;
}

int mbk_deep_orbit_read_wide(const mbk_deep_orbit *orbit, double *xr, double *xi, int32_t *xe, uint64_t n)
{
    if (!orbit || !xr || !xi || !xe) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    const uint64_t entries = (uint64_t)orbit->o.length + 1u;
    if (n < entries) return fail(nullptr, MBK_ERR_INVALID, "the output holds fewer than length + 1 entries");
    for (uint64_t k = 0; k < entries; ++k) {
        xr[k] = orbit->o.wide[k].xr;
        xi[k] = orbit->o.wide[k].xi;
        xe[k] = orbit->o.wide[k].xe;
    }
    return MBK_OK;
}

static const size_t kMaxDeepCopies = 8;

// This ctx's device copy of `orbit`, uploaded on first use.  A copy is never overwritten, and none is freed while a launch
// that reads it may still be queued: past kMaxDeepCopies copies the device is drained and all of them go (mbk.h).
// *out points into ctx->deep: good until the next call.
static int deep_copy(mbk_ctx *ctx, const mbk_deep_orbit *orbit, mbk_ctx::DeepCopy **out)
{
    for (mbk_ctx::DeepCopy &c : ctx->deep)
        if (c.id == orbit->o.id) {
            *out = &c;
            return MBK_OK;
        }
    if (ctx->capturing) return refuse_capture(ctx, "the reference orbit is not on the device, and its upload is synchronous: make the same call once outside the capture");
    if (ctx->deep.size() >= kMaxDeepCopies) {
        MBK_HIP(ctx, hipDeviceSynchronize());
        for (mbk_ctx::DeepCopy &c : ctx->deep) free_deep_copy(c);
        ctx->deep.clear();
    }
    const size_t bytes = orbit->o.table.size() * sizeof(double);
    double4 *d = nullptr;
    MBK_HIP(ctx, hipMalloc((void **)&d, bytes));
    const hipError_t e = hipMemcpy(d, orbit->o.table.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(ctx, MBK_ERR_HIP, std::string("hipMemcpy (reference orbit): ") + hipGetErrorString(e));
    }
    mbk_ctx::DeepCopy c = mbk_ctx::DeepCopy();
    c.id = orbit->o.id;
    c.d = d;
    ctx->deep.push_back(c);
    *out = &ctx->deep.back();
    return MBK_OK;
}

static int validate_deep(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd, uint32_t flags)
{
    return validate_deep_view(
        ctx, orbit, v, mrd, flags,
        [&]() -> int {
            if (flags & ~(MBK_WANT_COUNTS | MBK_WANT_BYTES | MBK_DEEP_BLA))
                return fail(ctx, MBK_ERR_INVALID, "deep views take MBK_WANT_COUNTS / MBK_WANT_BYTES / MBK_DEEP_BLA only (no kernel selection, no fp32)");
            if ((flags & MBK_DEEP_BLA) && orbit->o.length > (1u << 31))
                return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_BLA: the orbit is longer than 2^31 (the table's indices are 32 bits wide)");
            return MBK_OK;
        },
        [&]() -> int {
            if (!deep_ranges_within(v, 0x1p-960)) return fail(ctx, MBK_ERR_INVALID, "deep view ranges must be finite and lie in [2^-960, 4]");
            return MBK_OK;
        });
}

// what the deep kernels share: the orbit, the view's geometry and window, mrd (every other field zero)
static void fill_deep_args(mbk::DeepArgs &a, const double4 *d_orbit, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd)
{
    std::memset(&a, 0, sizeof(a));
    const std::vector<double> &t = orbit->o.table;
    a.orbit = d_orbit;
    a.z1 = make_double4(t[4], t[5], t[6], t[7]);
    a.M = orbit->o.length;
    fill_deep_window(a, v, mrd);
}

// dcmax of "Deep-zoom views with bilinear approximation": fl(|dc_r(column 0)| + |dc_i(row 0)|) of the FULL view
static double deep_dcmax(const mbk_deep_view *v)
{
    volatile double s = std::fabs(deep_dc(0u, v->width, v->range_r)) + std::fabs(deep_dc(0u, v->height, v->range_i));
    return s;
}

static uint64_t dcmax_key(double dcmax)
{
    uint64_t bits;
    std::memcpy(&bits, &dcmax, sizeof(bits));
    return bits;
}

// the resident table of `dcmax` beside the copy, or NULL
static mbk_ctx::BlaSlot *bla_find(mbk_ctx::DeepCopy *c, double dcmax)
{
    for (mbk_ctx::BlaSlot &b : c->bla)
        if (b.has && b.dcmax_bits == dcmax_key(dcmax)) return &b;
    return nullptr;
}

// This ctx's device copy of `orbit` (deep_copy) with the table of `dcmax` beside it.  A copy holds two tables (DESIGN.md "Two
// tables per orbit").  A table that is not resident is built on the host and uploaded, synchronously, into a free place or
// over the table asked for least recently -- never over `keep` --, and that only after the device has drained, since a launch
// that reads the table it replaces may still be queued (mbk.h).  *out and *table point into ctx->deep: good until the next
// call.  M >= 2.
static int bla_copy(mbk_ctx *ctx, const mbk_deep_orbit *orbit, double dcmax, const mbk_ctx::DeepCopy **out,
                    const mbk_ctx::BlaSlot **table, const mbk_ctx::BlaSlot *keep = nullptr)
{
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, orbit, &c);
    if (rc != MBK_OK) return rc;
    *out = c;
    mbk_ctx::BlaSlot *b = bla_find(c, dcmax);
    if (b) {
        b->used = ++c->bla_clock;
        *table = b;
        return MBK_OK;
    }
    if (ctx->capturing)
        return refuse_capture(ctx, "the bilinear-approximation table of this view's dcmax is not on the device, and it is built and uploaded synchronously: make the same call once outside the capture");
    for (mbk_ctx::BlaSlot &x : c->bla) {
        if (&x == keep) continue;
        if (!b || (b->has && (!x.has || x.used < b->used))) b = &x;
    }
    mbk::BlaTable t;
    try {
        mbk::build_bla_table(orbit->o.table, orbit->o.length, dcmax, &t);
    } catch (const std::bad_alloc &) {
        return fail(ctx, MBK_ERR_NOMEM, "out of host memory for the bilinear-approximation table");
    }
    if (b->has) MBK_HIP(ctx, hipDeviceSynchronize());
    b->has = false;
    // the sizes depend on M alone: allocated once per place
    if (!b->d_rc) MBK_HIP(ctx, hipMalloc((void **)&b->d_rc, t.rc.size() * sizeof(double)));
    if (!b->d_ab) MBK_HIP(ctx, hipMalloc((void **)&b->d_ab, t.rc.size() * sizeof(double4)));
    MBK_HIP(ctx, hipMemcpy(b->d_rc, t.rc.data(), t.rc.size() * sizeof(double), hipMemcpyHostToDevice));
    MBK_HIP(ctx, hipMemcpy(b->d_ab, t.ab.data(), t.ab.size() * sizeof(double), hipMemcpyHostToDevice));
    c->levels = t.levels;
    std::memcpy(c->off, t.off, sizeof(c->off));
    b->dcmax_bits = dcmax_key(dcmax);
    b->used = ++c->bla_clock;
    b->has = true;
    *table = b;
    return MBK_OK;
}

// the table of a launch in a kernel's arguments
static void fill_bla_table(mbk::DeepBlaArgs &a, const mbk_ctx::DeepCopy *c, const mbk_ctx::BlaSlot *table)
{
    a.rc = table->d_rc;
    a.ab = table->d_ab;
    a.levels = c->levels;
    std::memcpy(a.off, c->off, sizeof(a.off));
}

// the deep kernel on device pointers (validated by the caller), on `stream`; bla: MBK_DEEP_BLA (an orbit of length 1 has no
// table: the flag changes nothing)
static int launch_deep(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd,
                       int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, hipStream_t stream, bool bla = false)
{
    if (bla && orbit->o.length >= 2u) {
        const mbk_ctx::DeepCopy *c = nullptr;
        const mbk_ctx::BlaSlot *table = nullptr;
        int rc = bla_copy(ctx, orbit, deep_dcmax(v), &c, &table);
        if (rc != MBK_OK) return rc;
        mbk::DeepBlaArgs a;
        std::memset(&a, 0, sizeof(a));
        fill_deep_args(a.v, c->d, orbit, v, mrd);
        fill_outputs(a.v, mrd, d_counts, d_bytes, d_smooth);
        fill_bla_table(a, c, table);
        hipLaunchKernelGGL(mbk::deep_bla_kernel, block_grid(a.v), dim3(64), 0, stream, a);
        MBK_HIP(ctx, hipGetLastError());
        return MBK_OK;
    }
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, orbit, &c);
    if (rc != MBK_OK) return rc;
    mbk::DeepArgs a;
    fill_deep_args(a, c->d, orbit, v, mrd);
    fill_outputs(a, mrd, d_counts, d_bytes, d_smooth);
    hipLaunchKernelGGL(mbk::deep_view_kernel, block_grid(a), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- host twins of the bilinear-approximation table and step (mbk_deep_bla.h): no ctx, no device -------------------------

static int bla_host_table(const mbk_deep_orbit *orbit, const mbk_deep_view *view, mbk::BlaTable *t)
{
    int rc = validate_deep(nullptr, orbit, view, 0u, MBK_DEEP_BLA);
    if (rc != MBK_OK) return rc;
    try {
        mbk::build_bla_table(orbit->o.table, orbit->o.length, deep_dcmax(view), t);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, MBK_ERR_NOMEM, "out of host memory for the bilinear-approximation table");
    }
    return MBK_OK;
}

int mbk_deep_bla_info(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t *levels, uint64_t *entries)
{
    int rc = validate_deep(nullptr, orbit, view, 0u, MBK_DEEP_BLA);
    if (rc != MBK_OK) return rc;
    if (levels) *levels = mbk::bla_levels(orbit->o.length);
    if (entries) *entries = mbk::bla_entries(orbit->o.length);
    return MBK_OK;
}

int mbk_deep_bla_read(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t level, double *A_r, double *A_i,
                      double *B_r, double *B_i, double *rc_out, uint64_t n)
{
    if (!A_r || !A_i || !B_r || !B_i || !rc_out) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::BlaTable t;
    int rc = bla_host_table(orbit, view, &t);
    if (rc != MBK_OK) return rc;
    if (level >= t.levels) return fail(nullptr, MBK_ERR_INVALID, "the table has no such level");
    const uint32_t cnt = t.count(level);
    if (n < cnt) return fail(nullptr, MBK_ERR_INVALID, "the outputs hold fewer than the level's entries");
    for (uint32_t j = 0; j < cnt; ++j) {
        const size_t e = (size_t)t.off[level] + j;
        A_r[j] = t.ab[4 * e];
        A_i[j] = t.ab[4 * e + 1];
        B_r[j] = t.ab[4 * e + 2];
        B_i[j] = t.ab[4 * e + 3];
        rc_out[j] = t.rc[e];
    }
    return MBK_OK;
}

int mbk_deep_bla_count_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                            int32_t *count, double *mag, uint64_t *steps_executed)
{
    if (!count || !mag || !steps_executed) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::BlaTable t;
    int rc = bla_host_table(orbit, view, &t);
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(nullptr, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::bla_count_host(orbit->o.table, orbit->o.length, t, dc.r, dc.i,
                        (int64_t)mrd, count, mag, steps_executed);
    return MBK_OK;
}

// ---- extended-range deep views (mbk_deep_wide.h; mbk.h "Extended-range deep views") ----------------------------------------

// This ctx's device copy of `orbit` (deep_copy) with the wide table beside it, uploaded on the orbit's first wide launch here.
// Like the copy itself it is never overwritten and is freed with it.
static int wide_copy(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk::WideEntry **out)
{
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, orbit, &c);
    if (rc != MBK_OK) return rc;
    if (!c->d_wide) {
        if (ctx->capturing)
            return refuse_capture(ctx, "the wide reference orbit is not on the device, and its upload is synchronous: make the same call once outside the capture");
        const size_t bytes = orbit->o.wide.size() * sizeof(mbk::WideEntry);
        mbk::WideEntry *d = nullptr;
        MBK_HIP(ctx, hipMalloc((void **)&d, bytes));
        const hipError_t e = hipMemcpy(d, orbit->o.wide.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(ctx, MBK_ERR_HIP, std::string("hipMemcpy (wide reference orbit): ") + hipGetErrorString(e));
        }
        c->d_wide = d;
    }
    *out = c->d_wide;
    return MBK_OK;
}

static const char kNoWideBla[] = "MBK_DEEP_BLA is not implemented for extended-range deep views";   // (the count and the distance calls)

static int validate_deep_wide(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *v, uint32_t mrd, uint32_t flags)
{
    return validate_deep_view(
        ctx, orbit, v, mrd, flags,
        [&]() -> int {
            if (flags & MBK_DEEP_BLA) return fail(ctx, MBK_ERR_INVALID, kNoWideBla);
            if (flags & ~(MBK_WANT_COUNTS | MBK_WANT_BYTES | MBK_DEEP_XBLA))
                return fail(ctx, MBK_ERR_INVALID, "extended-range deep views take MBK_WANT_COUNTS / MBK_WANT_BYTES only (no kernel selection, no fp32)");
            if ((flags & MBK_DEEP_XBLA) && orbit->o.length > (1u << 31))
                return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA: the orbit is longer than 2^31 (the table's indices are 32 bits wide)");
            return MBK_OK;
        },
        [&]() -> int {
            if (!deep_ranges_within(v, 0x1p-64))
                return fail(ctx, MBK_ERR_INVALID, "extended-range deep view ranges must be finite and lie in [2^-64, 4]");
            if (v->exp2 > 0 || v->exp2 < -8192) return fail(ctx, MBK_ERR_INVALID, "extended-range deep view exp2 must lie in [-8192, 0]");
            return MBK_OK;
        });
}

// what the wide kernels share: the wide orbit, exp2, the view's geometry and window, mrd (every other field zero)
static void fill_deep_wide_args(mbk::DeepWideArgs &a, const mbk::WideEntry *d_orbit, const mbk_deep_orbit *orbit, const mbk_deep_xview *v,
                                uint32_t mrd)
{
    std::memset(&a, 0, sizeof(a));
    a.orbit = d_orbit;
    a.z1 = orbit->o.wide[1];
    a.M = orbit->o.length;
    a.exp2 = v->exp2;
    fill_deep_window(a, v, mrd);
}

// dcmax of "Extended-range deep views with bilinear approximation": of the FULL view, normalised
static mbk::WideReal wide_view_dcmax(const mbk_deep_xview *v)
{
    return mbk::wide_dcmax(deep_dc(0u, v->width, v->range_r), deep_dc(0u, v->height, v->range_i), v->exp2);
}

// the resident wide table of `dcmax` beside the copy, or NULL
static mbk_ctx::XblaSlot *xbla_find(mbk_ctx::DeepCopy *c, const mbk::WideReal &dcmax)
{
    for (mbk_ctx::XblaSlot &b : c->xbla)
        if (b.has && b.dcmax_bits == dcmax_key(dcmax.f) && b.dcmax_exp == dcmax.e) return &b;
    return nullptr;
}

// This ctx's device copy of `orbit` with its wide table (wide_copy) and the wide bilinear-approximation table of `dcmax`
// beside it: bla_copy's rule.  A copy holds two tables, keyed by dcmax's mantissa bits and exponent.  A table that is not
// resident is built on the host and uploaded, synchronously, into a free place or over the table asked for least recently --
// never over `keep` --, and that only after the device has drained, since a launch that reads the table it replaces may still
// be queued (mbk.h).  The second place is allocated when a second dcmax arrives.  *out and *table point into ctx->deep: good
// until the next call.  M >= 2.
static int xbla_copy(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk::WideReal &dcmax, const mbk_ctx::DeepCopy **out,
                     const mbk_ctx::XblaSlot **table, const mbk_ctx::XblaSlot *keep = nullptr)
{
    const mbk::WideEntry *d_orbit = nullptr;
    int rc = wide_copy(ctx, orbit, &d_orbit);
    if (rc != MBK_OK) return rc;
    mbk_ctx::DeepCopy *c = nullptr;
    rc = deep_copy(ctx, orbit, &c);
    if (rc != MBK_OK) return rc;
    *out = c;
    mbk_ctx::XblaSlot *b = xbla_find(c, dcmax);
    if (b) {
        b->used = ++c->xbla_clock;
        *table = b;
        return MBK_OK;
    }
    if (ctx->capturing)
        return refuse_capture(ctx, "the wide bilinear-approximation table of this view's dcmax is not on the device, and it is built and uploaded synchronously: make the same call once outside the capture");
    for (mbk_ctx::XblaSlot &x : c->xbla) {
        if (&x == keep) continue;
        if (!b || (b->has && (!x.has || x.used < b->used))) b = &x;
    }
    mbk::WideBlaTable t;
    try {
        mbk::build_wide_bla_table(orbit->o.wide, orbit->o.length, dcmax, &t);
    } catch (const std::bad_alloc &) {
        return fail(ctx, MBK_ERR_NOMEM, "out of host memory for the wide bilinear-approximation table");
    }
    if (b->has) MBK_HIP(ctx, hipDeviceSynchronize());
    b->has = false;
    // the sizes depend on M alone: allocated once per place
    if (!b->d_ke) MBK_HIP(ctx, hipMalloc((void **)&b->d_ke, t.ke.size() * sizeof(int32_t)));
    if (!b->d_ab) MBK_HIP(ctx, hipMalloc((void **)&b->d_ab, t.ab.size() * sizeof(mbk::WideBlaEntry)));
    MBK_HIP(ctx, hipMemcpy(b->d_ke, t.ke.data(), t.ke.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MBK_HIP(ctx, hipMemcpy(b->d_ab, t.ab.data(), t.ab.size() * sizeof(mbk::WideBlaEntry), hipMemcpyHostToDevice));
    c->xlevels = t.levels;
    std::memcpy(c->xoff, t.off, sizeof(c->xoff));
    b->dcmax_bits = dcmax_key(dcmax.f);
    b->dcmax_exp = dcmax.e;
    b->used = ++c->xbla_clock;
    b->has = true;
    *table = b;
    return MBK_OK;
}

// the table of a launch in a wide kernel's arguments
static void fill_xbla_table(mbk::DeepWideBlaArgs &a, const mbk_ctx::DeepCopy *c, const mbk_ctx::XblaSlot *table)
{
    a.ke = table->d_ke;
    a.ab = table->d_ab;
    a.levels = c->xlevels;
    std::memcpy(a.off, c->xoff, sizeof(a.off));
}

// the wide kernel on device pointers (validated by the caller), on `stream`; xbla: MBK_DEEP_XBLA (an orbit of length 1 has no
// table: the flag changes nothing)
static int launch_deep_wide(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *v, uint32_t mrd,
                            int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, hipStream_t stream, bool xbla = false)
{
    const mbk_ctx::DeepCopy *c = nullptr;
    const mbk_ctx::XblaSlot *slot = nullptr;
    const mbk::WideEntry *d_orbit = nullptr;
    const bool table = xbla && orbit->o.length >= 2u;
    int rc = table ? xbla_copy(ctx, orbit, wide_view_dcmax(v), &c, &slot) : wide_copy(ctx, orbit, &d_orbit);
    if (rc != MBK_OK) return rc;
    mbk::DeepWideBlaArgs b;
    std::memset(&b, 0, sizeof(b));
    mbk::DeepWideArgs &a = b.v;
    fill_deep_wide_args(a, table ? c->d_wide : d_orbit, orbit, v, mrd);
    fill_outputs(a, mrd, d_counts, d_bytes, d_smooth);
    if (table) {
        fill_xbla_table(b, c, slot);
        hipLaunchKernelGGL(mbk::deep_wide_bla_kernel, block_grid(a), dim3(64), 0, stream, b);
    } else {
        hipLaunchKernelGGL(mbk::deep_wide_kernel, block_grid(a), dim3(64), 0, stream, a);
    }
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- host twins of the wide bilinear-approximation table and step (mbk_deep_wide_bla.h): no ctx, no device ---------------

static int xbla_host_table(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, mbk::WideBlaTable *t)
{
    int rc = validate_deep_wide(nullptr, orbit, view, 0u, MBK_DEEP_XBLA);
    if (rc != MBK_OK) return rc;
    try {
        mbk::build_wide_bla_table(orbit->o.wide, orbit->o.length, wide_view_dcmax(view), t);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, MBK_ERR_NOMEM, "out of host memory for the wide bilinear-approximation table");
    }
    return MBK_OK;
}

int mbk_deep_xbla_info(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t *levels, uint64_t *entries)
{
    int rc = validate_deep_wide(nullptr, orbit, view, 0u, MBK_DEEP_XBLA);
    if (rc != MBK_OK) return rc;
    if (levels) *levels = mbk::bla_levels(orbit->o.length);
    if (entries) *entries = mbk::bla_entries(orbit->o.length);
    return MBK_OK;
}

int mbk_deep_xbla_read(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t level, double *A_r, double *A_i,
                       int32_t *a_e, double *B_r, double *B_i, int32_t *b_e, int32_t *ke, uint64_t n)
{
    if (!A_r || !A_i || !a_e || !B_r || !B_i || !b_e || !ke) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::WideBlaTable t;
    int rc = xbla_host_table(orbit, view, &t);
    if (rc != MBK_OK) return rc;
    if (level >= t.levels) return fail(nullptr, MBK_ERR_INVALID, "the table has no such level");
    const uint32_t cnt = t.count(level);
    if (n < cnt) return fail(nullptr, MBK_ERR_INVALID, "the outputs hold fewer than the level's entries");
    for (uint32_t j = 0; j < cnt; ++j) {
        const size_t at = (size_t)t.off[level] + j;
        const mbk::WideBlaEntry &e = t.ab[at];
        A_r[j] = e.ar;
        A_i[j] = e.ai;
        a_e[j] = e.ae;
        B_r[j] = e.br;
        B_i[j] = e.bi;
        b_e[j] = e.be;
        ke[j] = t.ke[at];
    }
    return MBK_OK;
}

int mbk_deep_xbla_count_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                             int32_t *count, double *mag, uint64_t *steps_executed)
{
    if (!count || !mag || !steps_executed) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::WideBlaTable t;
    int rc = xbla_host_table(orbit, view, &t);
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(nullptr, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::wide_bla_count_host(orbit->o.wide, orbit->o.length, t, dc.r, dc.i, view->exp2, (int64_t)mrd, count, mag, steps_executed);
    return MBK_OK;
}

// host twin of the wide step (mbk_deep_wide.h): no ctx, no device
int mbk_deep_xview_count_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                              int32_t *count, double *mag)
{
    if (!count || !mag) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = validate_deep_wide(nullptr, orbit, view, mrd, 0u);
    if (rc != MBK_OK) return rc;
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::wide_count_host(orbit->o.wide, orbit->o.length, dc.r, dc.i,
                         view->exp2, (int64_t)mrd, count, mag);
    return MBK_OK;
}

// ---- distance estimates for deep views (mbk_deep_distance.h; mbk.h "Distance estimates for deep views") ----------------

// the deep distance kernel on device pointers (validated by the caller), on `stream`
static int launch_deep_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd,
                                int32_t *d_counts, double *d_rel, hipStream_t stream)
{
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, orbit, &c);
    if (rc != MBK_OK) return rc;
    mbk::DeepDistanceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_args(a.v, c->d, orbit, v, mrd);
    a.v.counts = d_counts;
    a.range_r = v->range_r;
    a.rel = d_rel;
    hipLaunchKernelGGL(mbk::deep_distance_kernel, block_grid(a.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

double mbk_deep_distance_value_host(double mag, double dmagD, int32_t e, double range_r, int32_t count)
{
    return mbk::deep_distance_value(mag, dmagD, e, range_r, count);
}

// ---- atom periods and Newton seeds of deep views (mbk_deep_nucleus.h; mbk.h "Locating minibrots in deep views") ----------

// the nucleus kernel on device pointers (validated by the caller), on `stream`
static int launch_deep_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd,
                               int32_t *d_counts, int32_t *d_period, double *d_delta, hipStream_t stream)
{
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, orbit, &c);
    if (rc != MBK_OK) return rc;
    mbk::DeepNucleusArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_args(a.v, c->d, orbit, v, mrd);
    a.v.counts = d_counts;
    a.range_r = v->range_r;
    a.period = d_period;
    a.delta = d_delta;
    hipLaunchKernelGGL(mbk::deep_nucleus_kernel, block_grid(a.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// Everything a nucleus call can refuse, before anything is allocated, enqueued or written.
static int deep_nucleus_check(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                              const void *period, const void *delta)
{
    if (!period || !delta) return fail(ctx, MBK_ERR_INVALID, "NULL period or delta pointer");
    if (flags & MBK_DEEP_BLA)
        return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_BLA is not implemented for atom periods (a skipped run has no |z_n| to compare)");
    if (flags) return fail(ctx, MBK_ERR_INVALID, "atom periods take no flags (no kernel selection, no fp32)");
    return validate_deep(ctx, orbit, view, mrd, 0u);
}

int mbk_deep_view_launch_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                 uint32_t flags, int32_t *d_counts, int32_t *d_period, double *d_delta, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = deep_nucleus_check(ctx, orbit, view, mrd, flags, d_period, d_delta);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_deep_nucleus(ctx, orbit, view, mrd, d_counts, d_period, d_delta, (hipStream_t)hip_stream);
}

int mbk_deep_view_compute_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                  uint32_t flags, int32_t *h_counts, int32_t *h_period, double *h_delta, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = deep_nucleus_check(ctx, orbit, view, mrd, flags, h_period, h_delta);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    // the device values: 2 px binary64 (delta), then px int32 (the periods)
    const size_t px = (size_t)view->ncols * view->nrows;
    return compute_values(
        ctx, px, mrd, h_counts, h_delta, stats,
        [&](int32_t *d_counts, double *d_delta, hipStream_t stream) {
            return launch_deep_nucleus(ctx, orbit, view, mrd, d_counts, reinterpret_cast<int32_t *>(d_delta + 2u * px), d_delta, stream);
        },
        true, h_period, 2u);
}

// host twins (mbk_deep_nucleus.h): no ctx, no device
int mbk_deep_nucleus_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                          int32_t *count, int32_t *period, double *best, double *z_b, double *D_b, int32_t *e_b, double *delta)
{
    if (!count || !period || !best || !z_b || !D_b || !e_b || !delta) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = validate_deep(nullptr, orbit, view, mrd, 0u);
    if (rc != MBK_OK) return rc;
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::NucleusBest b;
    mbk::deep_nucleus_host(orbit->o.table, orbit->o.length, dc.r, dc.i, view->range_r, (int64_t)mrd, count, &b, delta);
    *period = b.arg + 1;
    *best = b.best;
    z_b[0] = b.zr;
    z_b[1] = b.zi;
    D_b[0] = b.Dr;
    D_b[1] = b.Di;
    *e_b = b.e;
    return MBK_OK;
}

static int orbit_period_check(const mbk_deep_orbit *orbit, uint32_t period, const void *a, const void *b, const void *c)
{
    if (!orbit || !a || !b || !c) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    if (period == 0u) return fail(nullptr, MBK_ERR_INVALID, "period must be >= 1");
    if (orbit->o.length < period) return fail(nullptr, MBK_ERR_INVALID, "the orbit is shorter than the period");
    return MBK_OK;
}

int mbk_deep_orbit_newton_host(const mbk_deep_orbit *orbit, uint32_t period, double *d_r, double *d_i, int32_t *d_e)
{
    int rc = orbit_period_check(orbit, period, d_r, d_i, d_e);
    if (rc != MBK_OK) return rc;
    const mbk::WideComplex w = mbk::wide_newton_step(orbit->o.wide, period);
    *d_r = w.r;
    *d_i = w.i;
    *d_e = w.e;
    return MBK_OK;
}

int mbk_deep_orbit_size_host(const mbk_deep_orbit *orbit, uint32_t period, double *s_r, double *s_i, int32_t *s_e)
{
    int rc = orbit_period_check(orbit, period, s_r, s_i, s_e);
    if (rc != MBK_OK) return rc;
    const mbk::WideComplex w = mbk::wide_size_estimate(orbit->o.wide, period);
    *s_r = w.r;
    *s_i = w.i;
    *s_e = w.e;
    return MBK_OK;
}

// ---- the same from extended-range deep views (mbk_deep_wide_nucleus.h; mbk.h "Locating minibrots in extended-range deep
// views") ------------------------------------------------------------------------------------------------------------------

// the wide nucleus kernel on device pointers (validated by the caller), on `stream`
static int launch_deep_wide_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *v, uint32_t mrd,
                                    int32_t *d_counts, int32_t *d_period, double *d_delta, hipStream_t stream)
{
    const mbk::WideEntry *d_orbit = nullptr;
    int rc = wide_copy(ctx, orbit, &d_orbit);
    if (rc != MBK_OK) return rc;
    mbk::DeepWideNucleusArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_wide_args(a.v, d_orbit, orbit, v, mrd);
    a.v.counts = d_counts;
    a.range_r = v->range_r;
    a.period = d_period;
    a.delta = d_delta;
    hipLaunchKernelGGL(mbk::deep_wide_nucleus_kernel, block_grid(a.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// Everything a wide nucleus call can refuse, before anything is allocated, enqueued or written.
static int wide_nucleus_check(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                              const void *period, const void *delta)
{
    if (!period || !delta) return fail(ctx, MBK_ERR_INVALID, "NULL period or delta pointer");
    if (flags & MBK_DEEP_XBLA)
        return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA is not implemented for atom periods (a skipped run has no |z_n| to compare)");
    if (flags & MBK_DEEP_BLA)
        return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_BLA is not implemented for extended-range deep views (and a skipped run has no |z_n| to compare)");
    if (flags) return fail(ctx, MBK_ERR_INVALID, "extended-range atom periods take no flags (no kernel selection, no fp32)");
    return validate_deep_wide(ctx, orbit, view, mrd, 0u);
}

int mbk_deep_xview_launch_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                  uint32_t flags, int32_t *d_counts, int32_t *d_period, double *d_delta, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = wide_nucleus_check(ctx, orbit, view, mrd, flags, d_period, d_delta);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return launch_deep_wide_nucleus(ctx, orbit, view, mrd, d_counts, d_period, d_delta, (hipStream_t)hip_stream);
}

int mbk_deep_xview_compute_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                   uint32_t flags, int32_t *h_counts, int32_t *h_period, double *h_delta, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = wide_nucleus_check(ctx, orbit, view, mrd, flags, h_period, h_delta);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    // the device values: 2 px binary64 (delta), then px int32 (the periods)
    const size_t px = (size_t)view->ncols * view->nrows;
    return compute_values(
        ctx, px, mrd, h_counts, h_delta, stats,
        [&](int32_t *d_counts, double *d_delta, hipStream_t stream) {
            return launch_deep_wide_nucleus(ctx, orbit, view, mrd, d_counts, reinterpret_cast<int32_t *>(d_delta + 2u * px), d_delta, stream);
        },
        true, h_period, 2u);
}

// host twin (mbk_deep_wide_nucleus.h): no ctx, no device
int mbk_deep_xview_nucleus_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                                int32_t *count, int32_t *period, double *best_m, int32_t *best_e, double *z_b, int32_t *t_b, double *D_b,
                                int32_t *e_b, double *delta)
{
    if (!count || !period || !best_m || !best_e || !z_b || !t_b || !D_b || !e_b || !delta)
        return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = validate_deep_wide(nullptr, orbit, view, mrd, 0u);
    if (rc != MBK_OK) return rc;
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::WideNucleusBest b;
    mbk::wide_nucleus_host(orbit->o.wide, orbit->o.length, dc.r, dc.i, view->range_r, view->exp2, (int64_t)mrd, count, &b, delta);
    *period = b.arg + 1;
    *best_m = b.bm;
    *best_e = b.be;
    z_b[0] = b.zr;
    z_b[1] = b.zi;
    *t_b = b.t;
    D_b[0] = b.Dr;
    D_b[1] = b.Di;
    *e_b = b.e;
    return MBK_OK;
}

// ---- distance estimates for deep views with bilinear approximation (mbk_deep_distance_bla.h; mbk.h, the section of that
// name): the launch; the entry points follow the renders, below -----------------------------------------------------------

// the deep distance kernel that takes skips, on device pointers (validated by the caller), on `stream`: the table of the count
// launches (bla_copy); an orbit of length 1 has none and takes deep_distance_kernel
static int launch_deep_distance_bla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd,
                                    int32_t *d_counts, double *d_rel, hipStream_t stream)
{
    if (orbit->o.length < 2u) return launch_deep_distance(ctx, orbit, v, mrd, d_counts, d_rel, stream);
    const mbk_ctx::DeepCopy *c = nullptr;
    const mbk_ctx::BlaSlot *table = nullptr;
    int rc = bla_copy(ctx, orbit, deep_dcmax(v), &c, &table);
    if (rc != MBK_OK) return rc;
    mbk::DeepDistanceBlaArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_args(a.b.v, c->d, orbit, v, mrd);
    a.b.v.counts = d_counts;
    fill_bla_table(a.b, c, table);
    a.range_r = v->range_r;
    a.rel = d_rel;
    hipLaunchKernelGGL(mbk::deep_distance_bla_kernel, block_grid(a.b.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- relief shading for deep views (mbk_deep_relief.h; mbk.h "Relief shading for deep views"): the launch; the entry points
// follow the relief renders, below -------------------------------------------------------------------------------------------

// the one-pass deep relief kernel on device pointers (validated by the caller), on `stream`; d_counts, d_smooth and d_rel may be
// null.  bla: MBK_DEEP_BLA, on the table of the count launches (bla_copy); an orbit of length 1 has none and takes the plain kernel
static int launch_deep_relief(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *v, uint32_t mrd, bool bla,
                              int32_t *d_counts, double *d_normal, double *d_smooth, double *d_rel, hipStream_t stream)
{
    bla = bla && orbit->o.length >= 2u;
    const mbk_ctx::DeepCopy *c = nullptr;
    const mbk_ctx::BlaSlot *table = nullptr;
    int rc;
    if (bla) {
        rc = bla_copy(ctx, orbit, deep_dcmax(v), &c, &table);
    } else {
        mbk_ctx::DeepCopy *plain = nullptr;
        rc = deep_copy(ctx, orbit, &plain);
        c = plain;
    }
    if (rc != MBK_OK) return rc;
    mbk::DeepReliefArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_args(a.b.v, c->d, orbit, v, mrd);
    a.b.v.counts = d_counts;
    a.b.v.smooth = d_smooth;
    if (bla) fill_bla_table(a.b, c, table);
    a.range_r = v->range_r;
    a.normal = d_normal;
    a.rel = d_rel;
    if (bla) hipLaunchKernelGGL(mbk::deep_relief_bla_kernel, block_grid(a.b.v), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(mbk::deep_relief_kernel, block_grid(a.b.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- distance estimates for extended-range deep views (mbk_deep_wide_distance.h; mbk.h, the section of that name) -------

// the wide distance kernel on device pointers (validated by the caller), on `stream`
static int launch_deep_wide_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *v, uint32_t mrd,
                                     int32_t *d_counts, double *d_rel, hipStream_t stream)
{
    const mbk::WideEntry *d_orbit = nullptr;
    int rc = wide_copy(ctx, orbit, &d_orbit);
    if (rc != MBK_OK) return rc;
    mbk::DeepWideDistanceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_wide_args(a.v, d_orbit, orbit, v, mrd);
    a.v.counts = d_counts;
    a.range_r = v->range_r;
    a.rel = d_rel;
    hipLaunchKernelGGL(mbk::deep_wide_distance_kernel, block_grid(a.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// the wide distance kernel that takes skips, on device pointers (validated by the caller), on `stream`: the table of the
// MBK_DEEP_XBLA count launches (xbla_copy); an orbit of length 1 has none and takes deep_wide_distance_kernel
static int launch_deep_wide_distance_xbla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *v, uint32_t mrd,
                                          int32_t *d_counts, double *d_rel, hipStream_t stream)
{
    if (orbit->o.length < 2u) return launch_deep_wide_distance(ctx, orbit, v, mrd, d_counts, d_rel, stream);
    const mbk_ctx::DeepCopy *c = nullptr;
    const mbk_ctx::XblaSlot *slot = nullptr;
    int rc = xbla_copy(ctx, orbit, wide_view_dcmax(v), &c, &slot);
    if (rc != MBK_OK) return rc;
    mbk::DeepWideDistanceBlaArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_wide_args(a.b.v, c->d_wide, orbit, v, mrd);
    a.b.v.counts = d_counts;
    fill_xbla_table(a.b, c, slot);
    a.range_r = v->range_r;
    a.rel = d_rel;
    hipLaunchKernelGGL(mbk::deep_wide_distance_bla_kernel, block_grid(a.b.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- relief shading for extended-range deep views (mbk_deep_wide_relief.h; mbk.h, the section of that name): the launch; the
// entry points follow those of the deep views, below --------------------------------------------------------------------------

// the one-pass wide relief kernel on device pointers (validated by the caller), on `stream`; d_counts, d_smooth and d_rel may be
// null.  xbla: MBK_DEEP_XBLA, on the table of the count launches (xbla_copy: acquired before anything is enqueued); an orbit of
// length 1 has none and takes the plain kernel
static int launch_deep_wide_relief(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *v, uint32_t mrd, bool xbla,
                                   int32_t *d_counts, double *d_normal, double *d_smooth, double *d_rel, hipStream_t stream)
{
    xbla = xbla && orbit->o.length >= 2u;
    const mbk_ctx::DeepCopy *c = nullptr;
    const mbk_ctx::XblaSlot *slot = nullptr;
    const mbk::WideEntry *d_orbit = nullptr;
    int rc = xbla ? xbla_copy(ctx, orbit, wide_view_dcmax(v), &c, &slot) : wide_copy(ctx, orbit, &d_orbit);
    if (rc != MBK_OK) return rc;
    mbk::DeepWideReliefArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_deep_wide_args(a.b.v, xbla ? c->d_wide : d_orbit, orbit, v, mrd);
    a.b.v.counts = d_counts;
    a.b.v.smooth = d_smooth;
    if (xbla) fill_xbla_table(a.b, c, slot);
    a.range_r = v->range_r;
    a.normal = d_normal;
    a.rel = d_rel;
    if (xbla) hipLaunchKernelGGL(mbk::deep_wide_relief_xbla_kernel, block_grid(a.b.v), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(mbk::deep_wide_relief_kernel, block_grid(a.b.v), dim3(64), 0, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// host twins (mbk_deep_wide_distance.h): no ctx, no device
int mbk_deep_xview_distance_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                                 int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e, double *rel)
{
    if (!count || !extra || !mag || !D_r || !D_i || !e || !rel) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = validate_deep_wide(nullptr, orbit, view, mrd, 0u);
    if (rc != MBK_OK) return rc;
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::wide_distance_host(orbit->o.wide, orbit->o.length, dc.r, dc.i,
                            view->exp2, (int64_t)mrd, count, extra, mag, D_r, D_i, e);
    const double r2 = *D_r * *D_r, i2 = *D_i * *D_i;
    *rel = mbk::wide_distance_value(*mag, r2 + i2, *e, view->range_r, view->exp2, *count);
    return MBK_OK;
}

int mbk_deep_xdistance_step_host(double z_r, double z_i, int32_t t, double *D_r, double *D_i, int32_t *e)
{
    if (!D_r || !D_i || !e) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::wide_dstep(z_r, z_i, t, *D_r, *D_i, *e);
    return MBK_OK;
}

double mbk_deep_xdistance_value_host(double mag, double dmagD, int32_t e, double range_r, int32_t exp2, int32_t count)
{
    return mbk::wide_distance_value(mag, dmagD, e, range_r, exp2, count);
}

// ---- Julia views (mbk_julia.h; mbk.h "Julia views") ----------------------------------------------------------

// Everything a Julia launch can refuse, before anything is allocated, enqueued or written.  flags: MBK_WANT_* (MBK_WANT_BYTES:
// the launch produces bytes) and kernel selection.
static int julia_check(mbk_ctx *ctx, const mbk_view *v, double c_r, double c_i, uint32_t mrd, uint32_t flags)
{
    if (flags & ~(MBK_WANT_COUNTS | MBK_WANT_BYTES | MBK_KERNEL_MASK))
        return fail(ctx, MBK_ERR_INVALID, "Julia views take MBK_WANT_COUNTS / MBK_WANT_BYTES and kernel selection only (no fp32, no MBK_LAZY_UNIFORM)");
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if (kernel != MBK_KERNEL_DEFAULT && kernel != MBK_KERNEL_ASM && kernel != MBK_KERNEL_GROUP)
        return fail(ctx, MBK_ERR_INVALID, "Julia views are implemented by MBK_KERNEL_DEFAULT / _ASM / _GROUP only");
    if (!std::isfinite(c_r) || !std::isfinite(c_i)) return fail(ctx, MBK_ERR_INVALID, "the Julia parameter must be finite");
    bool dummy;
    int rc = validate_view(ctx, v, &dummy);
    if (rc != MBK_OK) return rc;
    if (mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    if ((flags & MBK_WANT_BYTES) && mrd == 0) return fail(ctx, MBK_ERR_INVALID, "mrd == 0 has no quantised form (division by zero)");
    return MBK_OK;
}

// the Julia kernel on device pointers (checked by the caller: julia_check), on `stream`.  The parameter is uniform, so the two
// exactness rules (mbk_julia.h) pick the instantiation here, once per launch.
static int launch_julia(mbk_ctx *ctx, const mbk_view *v, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                        int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, hipStream_t stream)
{
    mbk::JuliaArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.cr = c_r;
    a.ci = c_i;
    a.mrd = (int32_t)mrd;
    fill_outputs(a, mrd, d_counts, d_bytes, d_smooth);
    a.exact_steps = ctx->opt[MBK_OPT_EXACT_STEPS];
    a.cyc_window = ctx->opt[MBK_OPT_CYCLE_WINDOW];
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    const bool literal = mbk::julia_needs_literal(c_i);
    const bool per_step = kernel == MBK_KERNEL_ASM || literal || !mbk::julia_grouped_ok(c_r, c_i);
    const bool cyc = ctx->opt[MBK_OPT_CYCLE_DETECT] != 0u;
    const uint32_t gs = ctx->opt[MBK_OPT_GROUP_STEPS];
    const dim3 grid(a.blocks_x * ((v->nrows + 7u) / 8u)), block(64);
    // MBK_OPT_WAVE_LIMIT: unused dynamic LDS per workgroup.  The sizes were found on tile_asm_kernel, but a cap through LDS is a
    // property of the size alone: it admits at most 4 k workgroups per CU to any kernel, and this one's registers (at most 42
    // VGPRs: 8 waves per SIMD, 32 per CU) never bind before it.
    const uint32_t lds = ctx->wave_limit_lds[ctx->opt[MBK_OPT_WAVE_LIMIT] & 7u];
    if (literal)
        hipLaunchKernelGGL((mbk::julia_view_kernel<false, 0, false>), grid, block, lds, stream, a);
    else if (per_step)
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 0, false>), grid, block, lds, stream, a);
    else if (gs == 32u && !cyc)   // (with the cycle test 32 means 16: mbk_loops.inc)
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 32, false>), grid, block, lds, stream, a);
    else if (gs >= 16u && cyc)
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 16, true>), grid, block, lds, stream, a);
    else if (gs >= 16u)
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 16, false>), grid, block, lds, stream, a);
    else if (gs == 8u && cyc)
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 8, true>), grid, block, lds, stream, a);
    else if (gs == 8u)
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 8, false>), grid, block, lds, stream, a);
    else
        hipLaunchKernelGGL((mbk::julia_view_kernel<true, 4, false>), grid, block, lds, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// A checked launch (mbk_julia_distance.h).  Kernel "asm": one pass, the derivative rides in a per-step escape loop.  Every
// other selector: launch_julia with that selector writes the counts, then the derivative pass runs each escaped pixel for
// exactly its count.  The doubling is the count launch's (julia_needs_literal), so both passes walk the same z.
static int launch_julia_distance(mbk_ctx *ctx, const mbk_view *v, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                 int32_t *d_counts, double *d_distance, hipStream_t stream)
{
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    const bool one_pass = kernel == MBK_KERNEL_ASM;
    if (!one_pass) {
        int rc = launch_count_pass(ctx, (size_t)v->ncols * v->nrows, stream, &d_counts, [&](int32_t *counts) {
            return launch_julia(ctx, v, c_r, c_i, mrd, kernel, counts, nullptr, nullptr, stream);
        });
        if (rc != MBK_OK) return rc;
    }
    mbk::JuliaDistanceArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_window(a, v);
    a.blocks_x = (v->ncols + 7u) / 8u;
    a.cr = c_r;
    a.ci = c_i;
    a.mrd = (int32_t)mrd;
    a.counts_in = one_pass ? nullptr : d_counts;
    a.counts_out = one_pass ? d_counts : nullptr;
    a.distance = d_distance;
    const bool literal = mbk::julia_needs_literal(c_i);
    const dim3 grid(a.blocks_x * ((v->nrows + 7u) / 8u)), block(64);   // (at most 2^31 / 64 blocks: validate_view)
    if (one_pass) {
        if (literal) hipLaunchKernelGGL((mbk::julia_distance_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mbk::julia_distance_kernel<true, true>), grid, block, 0, stream, a);
    } else {
        if (literal) hipLaunchKernelGGL((mbk::julia_distance_kernel<false, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mbk::julia_distance_kernel<true, false>), grid, block, 0, stream, a);
    }
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// ---- the count calls of the deep, extended-range and Julia views, and what renders and histograms share with them --------

// Everything a sample launch on `t` can refuse, before anything is allocated, enqueued or written: the rules of the kind's own
// launch.  flags: the kind's flags and MBK_WANT_* for what the launch produces (MBK_WANT_BYTES: the quantised form).  A caller
// with flag or source rules of its own (renders, histograms) applies them first.
static int target_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    switch (t.kind) {
        case Target::kWide: return validate_deep_wide(ctx, t.orbit, t.has_view ? &t.wide : nullptr, mrd, flags);
        case Target::kDeep: return validate_deep(ctx, t.orbit, t.has_view ? &t.deep : nullptr, mrd, flags);
        case Target::kJulia: return julia_check(ctx, t.has_view ? &t.view : nullptr, t.c_r, t.c_i, mrd, flags);
        case Target::kPlain: break;
    }
    bool dummy;
    int rc = validate_view(ctx, t.has_view ? &t.view : nullptr, &dummy, (flags & MBK_PRECISION_F32) != 0);
    if (rc != MBK_OK) return rc;
    if (mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    if ((flags & MBK_WANT_BYTES) && mrd == 0) return fail(ctx, MBK_ERR_INVALID, "mrd == 0 has no quantised form (division by zero)");
    if ((flags & MBK_KERNEL_MASK) > MBK_KERNEL_SCAN) return fail(ctx, MBK_ERR_INVALID, "unknown MBK_KERNEL_* selector");
    return MBK_OK;
}

// Where a launch writes: each pointer may be null.  values: the smooth nu, or with `distance` the distance estimate of the
// kind (plain views: de; deep views: rel).
struct Outputs {
    int32_t *counts;
    uint8_t *bytes;
    double *values;
    bool distance;
    int32_t *period;   // interior views (plain views only): values is then the interior distance estimate
    bool interior;
    double *normals;   // relief (plain, deep and extended-range deep views): the normals of the samples, beside counts and nu
    double *rel;       // deep and extended-range deep normals: the distance estimate of the same final state, beside nu in `values`
    double *stripe;    // stripe renders (plain views only): the stripe averages of the samples, beside counts and nu
    uint32_t density, skip;
};

// The launch of a checked target (target_check) on device pointers, on `stream`: the one place that knows which kernels serve
// which kind.  flags: the kind's flags; the outputs say what is wanted.
static int target_launch(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const Outputs &o, hipStream_t stream)
{
    switch (t.kind) {
        case Target::kWide:
            if (o.normals)   // (one pass for counts, nu, normals and rel: a wide sample is paid once)
                return launch_deep_wide_relief(ctx, t.orbit, &t.wide, mrd, (flags & MBK_DEEP_XBLA) != 0, o.counts, o.normals, o.values, o.rel, stream);
            if (o.distance)   // (MBK_DEEP_XBLA reaches here from the _distance_xbla calls alone: every other distance call refuses it)
                return (flags & MBK_DEEP_XBLA) ? launch_deep_wide_distance_xbla(ctx, t.orbit, &t.wide, mrd, o.counts, o.values, stream)
                                               : launch_deep_wide_distance(ctx, t.orbit, &t.wide, mrd, o.counts, o.values, stream);
            return launch_deep_wide(ctx, t.orbit, &t.wide, mrd, o.counts, o.bytes, o.values, stream, (flags & MBK_DEEP_XBLA) != 0);
        case Target::kDeep:
            if (o.normals)   // (one pass for counts, nu, normals and rel: a deep sample is paid once)
                return launch_deep_relief(ctx, t.orbit, &t.deep, mrd, (flags & MBK_DEEP_BLA) != 0, o.counts, o.normals, o.values, o.rel, stream);
            if (o.distance)   // (MBK_DEEP_BLA reaches here from the _distance_bla calls alone: every public distance call refuses it)
                return (flags & MBK_DEEP_BLA) ? launch_deep_distance_bla(ctx, t.orbit, &t.deep, mrd, o.counts, o.values, stream)
                                              : launch_deep_distance(ctx, t.orbit, &t.deep, mrd, o.counts, o.values, stream);
            return launch_deep(ctx, t.orbit, &t.deep, mrd, o.counts, o.bytes, o.values, stream, (flags & MBK_DEEP_BLA) != 0);
        case Target::kJulia:
            if (o.distance)   // (reached from the Julia distance calls alone: mbk_julia_view_render_* refuses the source)
                return launch_julia_distance(ctx, &t.view, t.c_r, t.c_i, mrd, flags, o.counts, o.values, stream);
            return launch_julia(ctx, &t.view, t.c_r, t.c_i, mrd, flags, o.counts, o.bytes, o.values, stream);
        case Target::kPlain: break;
    }
    if (o.interior) {
        bool safe = false;
        int rc = interior_check(ctx, &t.view, mrd, flags, &safe);
        if (rc != MBK_OK) return rc;
        return launch_interior(ctx, &t.view, mrd, flags, safe, o.counts, o.period, o.values, stream);
    }
    if (o.distance) {
        bool safe = false;
        int rc = distance_check(ctx, &t.view, mrd, flags, &safe);
        if (rc != MBK_OK) return rc;
        return launch_distance(ctx, &t.view, mrd, flags, safe, o.counts, o.values, stream);
    }
    const uint32_t want = (o.counts ? MBK_WANT_COUNTS : 0u) | (o.bytes ? MBK_WANT_BYTES : 0u);
    int rc = launch_tile(ctx, &t.view, mrd, (flags & ~(MBK_WANT_COUNTS | MBK_WANT_BYTES)) | want, o.counts, o.bytes, stream, o.values);
    if (rc != MBK_OK || (!o.normals && !o.stripe)) return rc;
    bool safe = false;   // (a relief or stripe band: the two-pass kernel on the counts the smooth launch has just written)
    rc = validate_view(ctx, &t.view, &safe);
    if (rc != MBK_OK) return rc;
    if (o.stripe) return launch_stripe_kernel(ctx, &t.view, safe, o.density, o.skip, o.counts, o.stripe, nullptr, stream);
    return launch_relief_kernel(ctx, &t.view, mrd, safe, o.counts, nullptr, o.normals, nullptr, stream);
}

// The three forms of a count call on a target: device pointers on a stream, host pointers synchronously, host pointers on a slot.
static int target_view_launch(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, int32_t *d_counts, uint8_t *d_bytes,
                              double *d_smooth, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = target_check(ctx, t, mrd, flags);
    if (rc != MBK_OK) return rc;
    const bool wc = (flags & MBK_WANT_COUNTS) != 0, wb = (flags & MBK_WANT_BYTES) != 0;
    if (!wc && !wb && !d_smooth) return fail(ctx, MBK_ERR_INVALID, "flags and d_smooth select no output");
    rc = check_wanted(ctx, flags, d_counts, d_bytes);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return target_launch(ctx, t, mrd, flags, Outputs{wc ? d_counts : nullptr, wb ? d_bytes : nullptr, d_smooth, false}, (hipStream_t)hip_stream);
}

static int target_view_compute(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, int32_t *h_counts, uint8_t *h_bytes,
                               double *h_smooth, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = target_check(ctx, t, mrd, flags);
    if (rc != MBK_OK) return rc;
    return view_compute(ctx, (size_t)t.g.ncols * t.g.nrows, mrd, flags, h_counts, h_bytes, h_smooth, stats,
                        [&](int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, hipStream_t stream) {
                            return target_launch(ctx, t, mrd, flags, Outputs{d_counts, d_bytes, d_smooth, false}, stream);
                        });
}

static int target_view_submit(mbk_ctx *ctx, int slot, const Target &t, uint32_t mrd, uint32_t flags, int32_t *h_counts, uint8_t *h_bytes)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (slot < 0 || slot >= MBK_SLOTS) return fail(ctx, MBK_ERR_INVALID, "slot out of range");
    int rc = target_check(ctx, t, mrd, flags);
    if (rc != MBK_OK) return rc;
    return view_submit(ctx, slot, (size_t)t.g.ncols * t.g.nrows, mrd, flags, h_counts, h_bytes,
                       [&](int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, hipStream_t stream) {
                           return target_launch(ctx, t, mrd, flags, Outputs{d_counts, d_bytes, d_smooth, false}, stream);
                       });
}

int mbk_deep_view_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                         int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, void *hip_stream)
{
    return target_view_launch(ctx, deep_target(orbit, view), mrd, flags, d_counts, d_bytes, d_smooth, hip_stream);
}

int mbk_deep_view_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                          int32_t *h_counts, uint8_t *h_bytes, double *h_smooth, mbk_stats *stats)
{
    return target_view_compute(ctx, deep_target(orbit, view), mrd, flags, h_counts, h_bytes, h_smooth, stats);
}

int mbk_deep_view_submit(mbk_ctx *ctx, int slot, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                         uint32_t flags, int32_t *h_counts, uint8_t *h_bytes)
{
    return target_view_submit(ctx, slot, deep_target(orbit, view), mrd, flags, h_counts, h_bytes);
}

int mbk_deep_xview_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                          int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, void *hip_stream)
{
    return target_view_launch(ctx, wide_target(orbit, view), mrd, flags, d_counts, d_bytes, d_smooth, hip_stream);
}

int mbk_deep_xview_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                           int32_t *h_counts, uint8_t *h_bytes, double *h_smooth, mbk_stats *stats)
{
    return target_view_compute(ctx, wide_target(orbit, view), mrd, flags, h_counts, h_bytes, h_smooth, stats);
}

int mbk_deep_xview_submit(mbk_ctx *ctx, int slot, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                          uint32_t flags, int32_t *h_counts, uint8_t *h_bytes)
{
    return target_view_submit(ctx, slot, wide_target(orbit, view), mrd, flags, h_counts, h_bytes);
}

int mbk_julia_view_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                          int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, void *hip_stream)
{
    return target_view_launch(ctx, julia_target(view, c_r, c_i), mrd, flags, d_counts, d_bytes, d_smooth, hip_stream);
}

int mbk_julia_view_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                           int32_t *h_counts, uint8_t *h_bytes, double *h_smooth, mbk_stats *stats)
{
    return target_view_compute(ctx, julia_target(view, c_r, c_i), mrd, flags, h_counts, h_bytes, h_smooth, stats);
}

int mbk_julia_view_submit(mbk_ctx *ctx, int slot, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                          int32_t *h_counts, uint8_t *h_bytes)
{
    return target_view_submit(ctx, slot, julia_target(view, c_r, c_i), mrd, flags, h_counts, h_bytes);
}

int mbk_julia_count_host(double z_r, double z_i, double c_r, double c_i, uint32_t mrd, int32_t *count, double *mag)
{
    if (!count) return fail(nullptr, MBK_ERR_INVALID, "count is NULL");
    if (!std::isfinite(c_r) || !std::isfinite(c_i)) return fail(nullptr, MBK_ERR_INVALID, "the Julia parameter must be finite");
    if (mrd > 0x7fffffffu) return fail(nullptr, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    double m = 0.0;
    // the doubling a launch with this parameter would use (mbk_julia.h): both forms must give the contract's count.  A z_r beyond
    // what a view may hold (validate_view: 2^500) takes the literal form: fl(2 z_r) may overflow there, and with z_i = 0 the
    // literal inf * 0 is NaN where the fused form returns c_i.  Only z_0 can do that: a later |zr| >= 2^512 has mag = inf, escaped.
    const bool literal = mbk::julia_needs_literal(c_i) || !(std::fabs(z_r) <= kMaxCoord);
    *count = literal ? mbk::julia_count<false>(z_r, z_i, c_r, c_i, (int32_t)mrd, &m)
                     : mbk::julia_count<true>(z_r, z_i, c_r, c_i, (int32_t)mrd, &m);
    if (mag) *mag = m;
    return MBK_OK;
}

// ---- distance estimates for Julia views (mbk_julia_distance.h; mbk.h, the section of that name) ------------------------

int mbk_julia_distance_host(double z_r, double z_i, double c_r, double c_i, uint32_t mrd, int32_t *count, int32_t *extra,
                            double *zr, double *zi, double *dr, double *di, double *mag, double *dmag, double *de)
{
    if (!count) return fail(nullptr, MBK_ERR_INVALID, "count is NULL");
    if (!std::isfinite(c_r) || !std::isfinite(c_i)) return fail(nullptr, MBK_ERR_INVALID, "the Julia parameter must be finite");
    if (mrd > 0x7fffffffu) return fail(nullptr, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    // the doubling a launch with this parameter would use, and the literal one for a z_r no view can hold (mbk_julia_count_host)
    const bool literal = mbk::julia_needs_literal(c_i) || !(std::fabs(z_r) <= kMaxCoord);
    double d_r = 1.0, d_i = 0.0, m = 0.0;
    int32_t n = 0, x = 0;
    if (literal) mbk::julia_distance_orbit<false>(z_r, z_i, d_r, d_i, c_r, c_i, (int32_t)mrd, n, x, m);
    else mbk::julia_distance_orbit<true>(z_r, z_i, d_r, d_i, c_r, c_i, (int32_t)mrd, n, x, m);
    const double r2 = d_r * d_r, i2 = d_i * d_i;
    const double dm = r2 + i2;
    *count = n;
    if (extra) *extra = x;
    if (zr) *zr = z_r;
    if (zi) *zi = z_i;
    if (dr) *dr = d_r;
    if (di) *di = d_i;
    if (mag) *mag = m;
    if (dmag) *dmag = dm;
    if (de) *de = mbk::distance_value(m, dm, n);
    return MBK_OK;
}

// ---- rendering (mbk_render.h; mbk.h "Rendering") -----------------------------------------------------------

// equalized: the call carries a table (mbk_*_render_equalized_*, mbk_render_resolve_equalized_host): it takes
// MBK_RENDER_EQUALIZED and nothing else; the calls without a table refuse that source.
static int validate_render_spec(mbk_ctx *ctx, const mbk_render_spec *spec, bool equalized = false)
{
    if (!spec) return fail(ctx, MBK_ERR_INVALID, "render spec is NULL");
    if (!spec->palette) return fail(ctx, MBK_ERR_INVALID, "palette is NULL");
    const uint32_t s = spec->supersample;
    if (s != 1u && s != 2u && s != 3u && s != 4u && s != 8u) return fail(ctx, MBK_ERR_INVALID, "supersample must be 1, 2, 3, 4 or 8");
    if (equalized != (spec->source == MBK_RENDER_EQUALIZED))
        return fail(ctx, MBK_ERR_INVALID, equalized ? "the equalized calls take MBK_RENDER_EQUALIZED only"
                                                    : "MBK_RENDER_EQUALIZED needs a table: use the equalized calls");
    if (spec->source == MBK_RENDER_BYTES) {
        if (spec->palette_len != 256u) return fail(ctx, MBK_ERR_INVALID, "MBK_RENDER_BYTES takes a palette of 256 entries");
    } else if (spec->source == MBK_RENDER_SMOOTH || spec->source == MBK_RENDER_EQUALIZED) {
        if (spec->palette_len < 2u || spec->palette_len > 65536u)
            return fail(ctx, MBK_ERR_INVALID, "MBK_RENDER_SMOOTH / _EQUALIZED take a palette of 2 .. 65536 entries");
        if (!(spec->scale > 0.0) || !(spec->scale <= 0x1p20)) return fail(ctx, MBK_ERR_INVALID, "scale must lie in (0, 2^20]");
        if (!(std::fabs(spec->offset) <= 0x1p20)) return fail(ctx, MBK_ERR_INVALID, "offset must lie in [-2^20, 2^20]");
    } else if (spec->source == MBK_RENDER_DISTANCE || spec->source == MBK_RENDER_DISTANCE_REL) {
        if (spec->palette_len < 2u || spec->palette_len > 65536u)
            return fail(ctx, MBK_ERR_INVALID, "MBK_RENDER_DISTANCE / _DISTANCE_REL take a palette of 2 .. 65536 entries");
        if (!(spec->scale > 0.0) || !(spec->scale <= 0x1p80)) return fail(ctx, MBK_ERR_INVALID, "scale must lie in (0, 2^80]");
        if (!(std::fabs(spec->offset) <= 0x1p20)) return fail(ctx, MBK_ERR_INVALID, "offset must lie in [-2^20, 2^20]");
    } else {
        return fail(ctx, MBK_ERR_INVALID, "unknown MBK_RENDER_* source");
    }
    return MBK_OK;
}

static uint32_t pack_rgba(const uint8_t *c)
{
    return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
}

static mbk::RenderPalette render_palette(const mbk_render_spec *spec, const uint32_t *entries)
{
    mbk::RenderPalette p;
    p.entries = entries;
    p.n = spec->palette_len;
    p.n_rcp = 1.0 / (double)spec->palette_len;
    p.inside = pack_rgba(spec->inside);
    p.scale = spec->scale;
    p.offset = spec->offset;
    p.lut = nullptr;
    p.lut_mrd = 0u;
    p.unknown = p.outside = 0u;
    p.light_x = p.light_y = p.height = 0.0;
    p.stripe_lo = p.stripe_gain = 0.0;
    return p;
}

// An interior render inside the render machinery: its spec as an mbk_render_spec with a source of its own, which no public call
// lets through (validate_render_spec), and its two extra colours.
static const uint32_t kRenderSourceInterior = 0x100u;
struct InteriorColours { uint32_t unknown, outside; };
// A relief render inside the render machinery: an MBK_RENDER_SMOOTH spec, and the light it has no field for.
struct ReliefLight { double x, y, height; };
// A stripe render inside the render machinery: an MBK_RENDER_SMOOTH spec, and what it has no field for.
struct StripeShade { uint32_t density, skip; double lo, gain; };

// The stream's device palette: uploaded when it differs from what the device copy holds, after the launches that read that.
static int stream_palette(mbk_ctx *ctx, StreamScratch *sc, hipStream_t stream, const uint8_t *palette, uint32_t len)
{
    std::vector<uint32_t> words(len);
    for (uint32_t k = 0; k < len; ++k) words[k] = pack_rgba(palette + 4u * (size_t)k);
    if (ctx->capturing && (!sc->d_palette || words != sc->palette))
        return refuse_capture(ctx, "the palette differs from the one on the device, and its upload waits for the stream: make the same call once outside the capture");
    if (!sc->d_palette) MBK_HIP(ctx, hipMalloc((void **)&sc->d_palette, 65536u * sizeof(uint32_t)));
    if (words != sc->palette) {
        MBK_HIP(ctx, hipStreamSynchronize(stream));
        sc->palette.clear();
        MBK_HIP(ctx, hipMemcpy(sc->d_palette, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        sc->palette = words;
    }
    return MBK_OK;
}

// The equalisation table a call carries: lut_len == mrd + 2 entries, each finite and in [0, 1].
static int validate_lut(mbk_ctx *ctx, const double *h_lut, uint32_t lut_len, uint64_t mrd)
{
    if (!h_lut) return fail(ctx, MBK_ERR_INVALID, "equalisation table is NULL");
    if (mrd > MBK_HISTOGRAM_MAX_MRD) return fail(ctx, MBK_ERR_INVALID, "mrd exceeds MBK_HISTOGRAM_MAX_MRD");
    if ((uint64_t)lut_len != mrd + 2u) return fail(ctx, MBK_ERR_INVALID, "lut_len must equal mrd + 2");
    for (uint32_t k = 0; k < lut_len; ++k)
        if (!(h_lut[k] >= 0.0 && h_lut[k] <= 1.0))
            return fail(ctx, MBK_ERR_INVALID, "equalisation table entries must be finite and lie in [0, 1]");
    return MBK_OK;
}

// The stream's device copy of the table, under the palette's rule: uploaded when it differs, after the launches that read it.
static int stream_lut(mbk_ctx *ctx, StreamScratch *sc, hipStream_t stream, const double *h_lut, uint32_t lut_len)
{
    if (sc->lut.size() == lut_len && std::memcmp(sc->lut.data(), h_lut, (size_t)lut_len * sizeof(double)) == 0) return MBK_OK;
    if (ctx->capturing)
        return refuse_capture(ctx, "the equalisation table differs from the one on the device, and its upload waits for the stream: make the same call once outside the capture");
    MBK_HIP(ctx, hipStreamSynchronize(stream));
    sc->lut.clear();
    int rc = grow(ctx, sc->d_lut, sc->lut_cap, lut_len, (size_t)lut_len * sizeof(double));
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipMemcpy(sc->d_lut, h_lut, (size_t)lut_len * sizeof(double), hipMemcpyHostToDevice));
    sc->lut.assign(h_lut, h_lut + lut_len);
    return MBK_OK;
}

// What a render takes from each kind of view beyond the sample launch's own rules (target_check), by Target::Kind: the flags it
// passes on, and the text that refuses MBK_RENDER_DISTANCE / MBK_RENDER_DISTANCE_REL where the kind has no such estimate.
struct RenderRules {
    uint32_t flags;
    const char *bad_flags, *no_distance, *no_distance_rel;
};
static const RenderRules kRenderRules[4] = {
    {MBK_KERNEL_MASK | MBK_PRECISION_F32, "render flags carry kernel selection (and MBK_PRECISION_F32) only", nullptr,
     "MBK_RENDER_DISTANCE_REL is implemented for deep views only (plain views: MBK_RENDER_DISTANCE)"},
    {MBK_KERNEL_MASK, "Julia render flags carry kernel selection only", "MBK_RENDER_DISTANCE is implemented for Mandelbrot views only (no Julia renders)",
     "MBK_RENDER_DISTANCE_REL is implemented for deep views only (plain views: MBK_RENDER_DISTANCE)"},
    {MBK_DEEP_BLA, "deep renders take MBK_DEEP_BLA only (no kernel selection, no fp32)",
     "MBK_RENDER_DISTANCE is implemented for plain views only (no deep renders)", nullptr},
    {MBK_DEEP_XBLA, "extended-range deep renders take no flags (no MBK_DEEP_BLA, no kernel selection, no fp32)",
     "distance estimates are not implemented for extended-range deep views", "distance estimates are not implemented for extended-range deep views"},
};

// What every render refuses of its output and of the view's geometry at supersample s, before the rules of the sample launch
// see the samples: target_samples needs a view, spans that fit 32 bits and a window inside the view.
static int render_geometry_check(mbk_ctx *ctx, const Target &t, uint32_t s, const void *out)
{
    if (!out) return fail(ctx, MBK_ERR_INVALID, "output pointer is NULL");
    if (!t.has_view) return fail(ctx, MBK_ERR_INVALID, "view is NULL");
    if ((uint64_t)t.g.width * s > 0xffffffffull || (uint64_t)t.g.height * s > 0xffffffffull)
        return fail(ctx, MBK_ERR_INVALID, "width or height times supersample does not fit 32 bits");
    if ((uint64_t)t.g.col0 + t.g.ncols > t.g.width || (uint64_t)t.g.row0 + t.g.nrows > t.g.height)
        return fail(ctx, MBK_ERR_INVALID, "window exceeds the view");
    return MBK_OK;
}

// Everything a render can refuse, before anything is allocated, enqueued or written.
static int render_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                        const void *out, bool equalized = false, const double *h_lut = nullptr, uint32_t lut_len = 0u)
{
    int rc = validate_render_spec(ctx, spec, equalized);
    if (rc != MBK_OK) return rc;
    const uint32_t s = spec->supersample;
    rc = render_geometry_check(ctx, t, s, out);
    if (rc != MBK_OK) return rc;
    const bool dist = spec->source == MBK_RENDER_DISTANCE;
    const bool rel = spec->source == MBK_RENDER_DISTANCE_REL;
    const bool smooth = spec->source == MBK_RENDER_SMOOTH || dist || rel || equalized;   // (the distance samples obey the smooth launch's rules)
    const RenderRules &rules = kRenderRules[t.kind];
    if (dist && rules.no_distance) return fail(ctx, MBK_ERR_INVALID, rules.no_distance);
    if (rel && rules.no_distance_rel) return fail(ctx, MBK_ERR_INVALID, rules.no_distance_rel);
    if (flags & ~rules.flags) return fail(ctx, MBK_ERR_INVALID, rules.bad_flags);
    if ((flags & MBK_DEEP_BLA) && rel) return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_BLA is not implemented for deep distance estimates");
    rc = target_check(ctx, target_samples(t, s, t.g.col0, t.g.row0, t.g.ncols, t.g.nrows), mrd, flags | (smooth ? 0u : MBK_WANT_BYTES));
    if (rc != MBK_OK) return rc;
    // (what follows can be true of a plain view only: no other kind takes these flags)
    const bool f32 = (flags & MBK_PRECISION_F32) != 0;
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if ((smooth || f32) && (kernel == MBK_KERNEL_SIMPLE || kernel == MBK_KERNEL_REFILL))
        return fail(ctx, MBK_ERR_INVALID, "smooth colouring and MBK_PRECISION_F32 are implemented by the scan / asm / group kernels only");
    if (smooth && f32) return fail(ctx, MBK_ERR_INVALID, "smooth colouring is implemented in binary64 only");
    return equalized ? validate_lut(ctx, h_lut, lut_len, mrd) : MBK_OK;
}

static size_t round_up_256(size_t x) { return (x + 255u) & ~(size_t)255u; }

// A checked render (render_check) onto the device image d_out (ncols x nrows words), on `stream`.  stat: the slot whose
// reduction scratch adds up the statistics of the samples and whose ev_k1 marks the last resolve kernel (_compute), or NULL.
static int render_run(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                      uint32_t *d_out, hipStream_t stream, Slot *stat, const double *h_lut = nullptr, uint32_t lut_len = 0u,
                      const InteriorColours *interior = nullptr, const ReliefLight *relief = nullptr, const StripeShade *stripe = nullptr)
{
    const uint32_t s = spec->supersample;
    const bool dist = spec->source == MBK_RENDER_DISTANCE || spec->source == MBK_RENDER_DISTANCE_REL;   // (deep views: rel in place of de, the same colour rule)
    const bool eq = spec->source == MBK_RENDER_EQUALIZED;                  // (the smooth samples, coloured through the table)
    const bool smooth = spec->source == MBK_RENDER_SMOOTH || dist || eq || interior;   // (same sample layout: binary64 value | counts; interior: | periods)
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;

    // the palette: uploaded when it differs from what this stream's device copy holds, after the launches that read that
    rc = stream_palette(ctx, sc, stream, spec->palette, spec->palette_len);
    if (rc != MBK_OK) return rc;
    if (eq) {
        rc = stream_lut(ctx, sc, stream, h_lut, lut_len);
        if (rc != MBK_OK) return rc;
    }

    const BandPlan plan = band_plan(t.g.ncols, t.g.nrows, (uint64_t)s * s * (relief ? 28u : stripe ? 20u : (interior ? 16u : (smooth ? 12u : (stat ? 5u : 1u)))), spec->max_band_rows);
    const size_t cap_samples = plan.cap_px() * s * s;
    // layout: SMOOTH nu | counts (interior: de | counts | periods; relief: nu | counts | normals; stripe: nu | counts | v); BYTES counts (statistics only) | bytes
    const size_t off2 = smooth ? round_up_256(cap_samples * 8u) : (stat ? round_up_256(cap_samples * 4u) : 0u);
    const size_t off3 = off2 + round_up_256(cap_samples * 4u);   // (interior, relief and stripe only)
    const size_t need = relief ? off3 + cap_samples * 16u : stripe ? off3 + cap_samples * 8u : (interior ? off3 + cap_samples * 4u : off2 + (smooth ? cap_samples * 4u : cap_samples));
    rc = grow(ctx, sc->d_render, sc->render_cap, need, need);
    if (rc != MBK_OK) return rc;
    uint8_t *base = (uint8_t *)sc->d_render;
    const Outputs samples = {smooth ? (int32_t *)(base + off2) : (stat ? (int32_t *)base : nullptr), smooth ? nullptr : base + off2,
                             smooth ? (double *)base : nullptr, dist, interior ? (int32_t *)(base + off3) : nullptr, interior != nullptr,
                             relief ? (double *)(base + off3) : nullptr, nullptr, stripe ? (double *)(base + off3) : nullptr,
                             stripe ? stripe->density : 0u, stripe ? stripe->skip : 0u};
    const double *d_lut = eq ? sc->d_lut : nullptr;
    const uint32_t *d_palette = sc->d_palette;   // (sc may move when a launch below adds a stream's scratch: not used past here)

    const size_t lds = (size_t)spec->palette_len * sizeof(uint32_t);
    const bool use_lds = spec->palette_len <= mbk::kRenderLdsEntries && lds <= ctx->prop.sharedMemPerBlock;
    const uint32_t cus = (uint32_t)std::max(ctx->prop.multiProcessorCount, 1);
    const uint32_t wg_per_cu = use_lds ? (uint32_t)std::min<size_t>(8u, std::max<size_t>(1u, (160u << 10) / lds)) : 8u;

    return for_each_band(ctx, plan, samples.counts, (uint64_t)s * s, mrd, stream, stat, [&](uint32_t r, uint32_t c, uint32_t nr, uint32_t nc, bool) -> int {
        int rc = target_launch(ctx, target_samples(t, s, t.g.col0 + c, t.g.row0 + r, nc, nr), mrd, flags, samples, stream);
        if (rc != MBK_OK) return rc;
        mbk::RenderArgs a;
        std::memset(&a, 0, sizeof(a));
        a.counts = samples.counts;
        a.smooth = samples.values;
        a.period = samples.period;
        a.normal = samples.normals;
        a.stripe = samples.stripe;
        a.bytes = samples.bytes;
        a.out = d_out + (size_t)r * t.g.ncols + c;
        a.pitch = (uint64_t)nc * s;
        a.out_pitch = t.g.ncols;
        a.ncols = nc;
        a.nrows = nr;
        const uint32_t px_per_wg = mbk::kRenderThreads * (smooth ? 1u : mbk::kRenderBytesPx);
        a.chunks_x = (nc + px_per_wg - 1u) / px_per_wg;
        a.lds_palette = use_lds ? 1u : 0u;
        a.pal = render_palette(spec, d_palette);
        a.pal.lut = d_lut;
        a.pal.lut_mrd = eq ? lut_len - 2u : 0u;
        if (interior) {
            a.pal.unknown = interior->unknown;
            a.pal.outside = interior->outside;
        }
        if (relief) {
            a.pal.light_x = relief->x;
            a.pal.light_y = relief->y;
            a.pal.height = relief->height;
        }
        if (stripe) {
            a.pal.stripe_lo = stripe->lo;
            a.pal.stripe_gain = stripe->gain;
        }
        const uint64_t pieces = (uint64_t)a.chunks_x * nr;
        const dim3 grid((uint32_t)std::min<uint64_t>(pieces, (uint64_t)cus * wg_per_cu));
        if (interior)
            mbk::launch_resolve<true, mbk::kRuleInterior>(s, grid, use_lds ? lds : 0u, stream, a);
        else if (relief)
            mbk::launch_resolve<true, mbk::kRuleRelief>(s, grid, use_lds ? lds : 0u, stream, a);
        else if (stripe)
            mbk::launch_resolve<true, mbk::kRuleStripe>(s, grid, use_lds ? lds : 0u, stream, a);
        else if (dist)
            mbk::launch_resolve<true, mbk::kRuleDistance>(s, grid, use_lds ? lds : 0u, stream, a);
        else if (eq)
            mbk::launch_resolve<true, mbk::kRuleEqualized>(s, grid, use_lds ? lds : 0u, stream, a);
        else if (smooth)
            mbk::launch_resolve<true>(s, grid, use_lds ? lds : 0u, stream, a);
        else
            mbk::launch_resolve<false>(s, grid, use_lds ? lds : 0u, stream, a);
        MBK_HIP(ctx, hipGetLastError());
        return MBK_OK;
    });
}

// equalized (here and in render_compute): the call carries the table h_lut[lut_len] and takes MBK_RENDER_EQUALIZED only
static int render_launch(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                         uint8_t *d_rgba, void *hip_stream, bool equalized = false, const double *h_lut = nullptr,
                         uint32_t lut_len = 0u)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = render_check(ctx, t, mrd, flags, spec, d_rgba, equalized, h_lut, lut_len);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags, spec, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr, h_lut, lut_len);
}

// A checked render synchronously into a host image on slot 0: what follows the refusals of a *_render_compute call.
static int render_compute_checked(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                  uint8_t *h_rgba, mbk_stats *stats, const double *h_lut, uint32_t lut_len,
                                  const InteriorColours *interior = nullptr, const ReliefLight *relief = nullptr,
                                  const StripeShade *stripe = nullptr)
{
    int rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    const size_t px = (size_t)t.g.ncols * t.g.nrows;
    auto enqueue = [&]() -> int {
        int rc = grow(ctx, ctx->d_rgba, ctx->rgba_cap_px, px, px * sizeof(uint32_t));
        if (rc != MBK_OK) return rc;
        // the bands add their statistics up in the slot's reduction scratch: cleared once, here
        MBK_HIP(ctx, hipMemsetAsync(sl.d_red, 0, sizeof(ReduceSlot) * mbk::kReduceSlots, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
        rc = render_run(ctx, t, mrd, flags, spec, ctx->d_rgba, sl.stream, &sl, h_lut, lut_len, interior, relief, stripe);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_rgba, ctx->d_rgba, px * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    return sync_end(ctx, enqueue(), stats, false);
}

static int render_compute(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                          uint8_t *h_rgba, mbk_stats *stats, bool equalized = false, const double *h_lut = nullptr,
                          uint32_t lut_len = 0u)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = render_check(ctx, t, mrd, flags, spec, h_rgba, equalized, h_lut, lut_len);
    if (rc != MBK_OK) return rc;
    return render_compute_checked(ctx, t, mrd, flags, spec, h_rgba, stats, h_lut, lut_len);
}

int mbk_view_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                           uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, view_target(view), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_view_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                            uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, view_target(view), mrd, flags, spec, h_rgba, stats);
}

int mbk_deep_view_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, deep_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_deep_view_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                 uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, deep_target(orbit, view), mrd, flags, spec, h_rgba, stats);
}

int mbk_view_render_equalized_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                     const double *h_lut, uint32_t lut_len, uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, view_target(view), mrd, flags, spec, d_rgba, hip_stream, true, h_lut, lut_len);
}

int mbk_view_render_equalized_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                      const double *h_lut, uint32_t lut_len, uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, view_target(view), mrd, flags, spec, h_rgba, stats, true, h_lut, lut_len);
}

int mbk_deep_view_render_equalized_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                          uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, deep_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream, true, h_lut, lut_len);
}

int mbk_deep_view_render_equalized_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                           uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, deep_target(orbit, view), mrd, flags, spec, h_rgba, stats, true, h_lut, lut_len);
}

int mbk_deep_xview_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                 uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, wide_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_deep_xview_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                  uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, wide_target(orbit, view), mrd, flags, spec, h_rgba, stats);
}

int mbk_deep_xview_render_equalized_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                           uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, wide_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream, true, h_lut, lut_len);
}

int mbk_deep_xview_render_equalized_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                            uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                            uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, wide_target(orbit, view), mrd, flags, spec, h_rgba, stats, true, h_lut, lut_len);
}

int mbk_julia_view_render_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                 const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return render_launch(ctx, julia_target(view, c_r, c_i), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_julia_view_render_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                  const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return render_compute(ctx, julia_target(view, c_r, c_i), mrd, flags, spec, h_rgba, stats);
}

int mbk_julia_view_render_equalized_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                           const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len, uint8_t *d_rgba,
                                           void *hip_stream)
{
    return render_launch(ctx, julia_target(view, c_r, c_i), mrd, flags, spec, d_rgba, hip_stream, true, h_lut, lut_len);
}

int mbk_julia_view_render_equalized_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                            const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len, uint8_t *h_rgba,
                                            mbk_stats *stats)
{
    return render_compute(ctx, julia_target(view, c_r, c_i), mrd, flags, spec, h_rgba, stats, true, h_lut, lut_len);
}

// jet as matplotlib defines it (a public piecewise-linear colour map; the reference's Viewer looks colours up in its 256-entry
// table): entry i of the table of a channel with knots (x, y), built the way LinearSegmentedColormap builds it -- positions
// 255 fl(i fl(1 / 255)), the first knot at or beyond one, and a linear step between that knot and the one before, every
// operation rounded on its own.
struct JetKnot { double x, y; };
static double jet_entry(const JetKnot *k, int m, int i)
{
    if (i == 0) return k[0].y;
    if (i == 255) return k[m - 1].y;
    const double step = 1.0 / 255.0;
    const double xi = 255.0 * ((double)i * step);
    int j = 1;
    while (j < m - 1 && k[j].x * 255.0 < xi) ++j;
    const double xa = k[j - 1].x * 255.0, xb = k[j].x * 255.0;
    const double d = (xi - xa) / (xb - xa);
    const double v = d * (k[j].y - k[j - 1].y) + k[j - 1].y;
    return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

int mbk_palette_viewer(uint8_t out[1024])
{
    if (!out) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    static const JetKnot red[] = {{0.0, 0.0}, {0.35, 0.0}, {0.66, 1.0}, {0.89, 1.0}, {1.0, 0.5}};
    static const JetKnot green[] = {{0.0, 0.0}, {0.125, 0.0}, {0.375, 1.0}, {0.64, 1.0}, {0.91, 0.0}, {1.0, 0.0}};
    static const JetKnot blue[] = {{0.0, 0.5}, {0.11, 1.0}, {0.34, 1.0}, {0.65, 0.0}, {1.0, 0.0}};
    // Viewer.py:110-135: v = 1 - b / 256 (exact), black where v == 1, else jet(v), whose table index is
    // min(int(256 v), 255) = 256 - b for b >= 1
    out[0] = out[1] = out[2] = 0u;
    out[3] = 255u;
    for (int b = 1; b < 256; ++b) {
        const int i = 256 - b;
        const double ch[4] = {jet_entry(red, 5, i), jet_entry(green, 6, i), jet_entry(blue, 5, i), 1.0};
        for (int c = 0; c < 4; ++c) out[4 * b + c] = (uint8_t)std::floor(255.0 * ch[c] + 0.5);
    }
    return MBK_OK;
}

// mbk_render_resolve_host, and with a table (equalized) mbk_render_resolve_equalized_host
static int resolve_host(const mbk_render_spec *spec, bool equalized, const double *h_lut, uint32_t lut_len, uint32_t width,
                        uint32_t height, const int32_t *counts, const uint8_t *bytes, const double *smooth, uint8_t *rgba)
{
    int rc = validate_render_spec(nullptr, spec, equalized);
    if (rc != MBK_OK) return rc;
    if (equalized) {
        if (lut_len < 2u) return fail(nullptr, MBK_ERR_INVALID, "lut_len must be mrd + 2");
        rc = validate_lut(nullptr, h_lut, lut_len, (uint64_t)lut_len - 2u);
        if (rc != MBK_OK) return rc;
    }
    if (!rgba) return fail(nullptr, MBK_ERR_INVALID, "output pointer is NULL");
    const uint32_t s = spec->supersample;
    if (width == 0 || height == 0 || (uint64_t)width * s >= (1ull << 31) || (uint64_t)height * s >= (1ull << 31))
        return fail(nullptr, MBK_ERR_INVALID, "width and height must be > 0 and, times supersample, below 2^31");
    const bool dist = spec->source == MBK_RENDER_DISTANCE || spec->source == MBK_RENDER_DISTANCE_REL;
    const bool sm = spec->source == MBK_RENDER_SMOOTH || dist || equalized;
    if (sm ? (!counts || !smooth) : !bytes) return fail(nullptr, MBK_ERR_INVALID, "the source's sample arrays are NULL");
    std::vector<uint32_t> words(spec->palette_len);
    for (uint32_t k = 0; k < spec->palette_len; ++k) words[k] = pack_rgba(spec->palette + 4u * (size_t)k);
    mbk::RenderPalette pal = render_palette(spec, words.data());
    pal.lut = h_lut;
    pal.lut_mrd = equalized ? lut_len - 2u : 0u;
    mbk::render_resolve_host(pal, sm, s, width, height, counts, bytes, smooth, rgba,
                             dist ? mbk::kRuleDistance : (equalized ? mbk::kRuleEqualized : mbk::kRuleSmooth));
    return MBK_OK;
}

int mbk_render_resolve_host(const mbk_render_spec *spec, uint32_t width, uint32_t height, const int32_t *counts,
                            const uint8_t *bytes, const double *smooth, uint8_t *rgba)
{
    return resolve_host(spec, false, nullptr, 0u, width, height, counts, bytes, smooth, rgba);
}

int mbk_render_resolve_equalized_host(const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len, uint32_t width,
                                      uint32_t height, const int32_t *counts, const double *smooth, uint8_t *rgba)
{
    return resolve_host(spec, true, h_lut, lut_len, width, height, counts, nullptr, smooth, rgba);
}

// ---- adaptive supersampling (mbk.h "Adaptive supersampling", "Adaptive supersampling of deep views" and "Adaptive
// supersampling of extended-range deep views"; mbk_adaptive.h, mbk_deep_adaptive.h, mbk_deep_wide_adaptive.h): plain, deep and
// extended-range deep views, MBK_RENDER_SMOOTH -------------------------------------------------------------------------------

// Everything an adaptive render can refuse, before anything is allocated, enqueued or written: its own rules, then the smooth
// render's for the sample view at s (render_check) and the sample launch's for the base samples of the output window: the base
// samples are launched per band of that window's halo, and the whole view -- which may hold far more than the 2^31 pixels of a
// window -- is never a launch.
static int adaptive_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                          uint32_t threshold, const void *out)
{
    if (spec && spec->source != MBK_RENDER_SMOOTH)
        return fail(ctx, MBK_ERR_INVALID, "adaptive supersampling is implemented for MBK_RENDER_SMOOTH only");
    if (threshold > 256u) return fail(ctx, MBK_ERR_INVALID, "threshold must lie in [0, 256]");
    if (t.kind == Target::kDeep && (flags & MBK_DEEP_XBLA))
        return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA belongs to extended-range deep views, which adaptive supersampling does not cover (a deep view takes MBK_DEEP_BLA)");
    int rc;
    if (t.kind == Target::kWide && (flags & MBK_DEEP_BLA)) {   // refused in validate_deep_wide's words, not the render rules'
        rc = target_check(ctx, t, mrd, flags);
        if (rc != MBK_OK) return rc;
    }
    rc = render_check(ctx, t, mrd, flags, spec, out);
    if (rc != MBK_OK) return rc;
    return target_check(ctx, target_samples(t, 1u, t.g.col0, t.g.row0, t.g.ncols, t.g.nrows), mrd, flags);
}

// The bands of an adaptive render: per band the base samples of its halo (12 bytes each, the band grown by one pixel on each
// side) and the list (4 bytes per pixel of the band) fit MBK_RENDER_BAND_BYTES beside the two counters.
static BandPlan adaptive_band_plan(uint32_t ncols, uint32_t nrows, uint32_t max_rows)
{
    const uint64_t budget = MBK_RENDER_BAND_BYTES - 2048u;   // (the parts of the scratch start on 256-byte lines)
    const uint64_t halo_row = ((uint64_t)ncols + 2u) * 12u, row = halo_row + (uint64_t)ncols * 4u;
    BandPlan p = {ncols, nrows, ncols, 1u};
    if (2u * halo_row + row <= budget) {
        // (bands of equal height: 4096 rows that miss the budget by the halo become 2 x 2048, not 4094 + 2)
        const uint32_t fit = (uint32_t)std::min<uint64_t>(nrows, (budget - 2u * halo_row) / row), bands = (nrows + fit - 1u) / fit;
        p.band_rows = (nrows + bands - 1u) / bands;
    } else
        p.tile_cols = (uint32_t)((budget - 72u) / 40u);   // 3 (tile_cols + 2) 12 + 4 tile_cols <= budget
    if (max_rows) p.band_rows = std::min(p.band_rows, max_rows);
    return p;
}

// The refine kernel's table of an adaptive render, copied out of the ctx (adaptive_tables): deep.rc / wide.ke stay NULL where
// the refine kernel takes the plain step or does not run.
struct AdaptiveFine {
    mbk::DeepBlaArgs deep;         // kDeep, MBK_DEEP_BLA
    mbk::DeepWideBlaArgs wide;     // kWide, MBK_DEEP_XBLA
};

// The tables of a checked adaptive render of a deep view with MBK_DEEP_BLA, or of an extended-range deep view with
// MBK_DEEP_XBLA, acquired TOGETHER before the render enqueues anything: the base pass steps with the table of the W x H view's
// dcmax, the refine kernel with that of the (W s) x (H s) view's, and neither may take the other's place (bla_copy's and
// xbla_copy's `keep`); equal dcmax are one table.  Once both are resident this finds them and waits for nothing.  fine: the
// refine kernel's table, copied out of the ctx; the pointers stay NULL where the refine kernel takes the plain step (no flag, an
// orbit of length 1) or does not run (s = 1, threshold 256: the base pass looks its own table up, as every deep launch does).
static int adaptive_tables(mbk_ctx *ctx, const Target &t, uint32_t flags, uint32_t s, uint32_t threshold, AdaptiveFine *fine)
{
    std::memset(fine, 0, sizeof(*fine));
    const bool deep = t.kind == Target::kDeep && (flags & MBK_DEEP_BLA), wide = t.kind == Target::kWide && (flags & MBK_DEEP_XBLA);
    if ((!deep && !wide) || t.orbit->o.length < 2u || s == 1u || threshold == 256u) return MBK_OK;
    const Target b = target_samples(t, 1u, 0u, 0u, t.g.width, t.g.height), f = target_samples(t, s, 0u, 0u, t.g.width, t.g.height);
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, t.orbit, &c);
    if (rc != MBK_OK) return rc;
    const mbk_ctx::DeepCopy *cc = nullptr;
    if (wide) {
        const mbk::WideReal dc_base = wide_view_dcmax(&b.wide), dc_fine = wide_view_dcmax(&f.wide);
        const mbk_ctx::XblaSlot *tb = nullptr, *tf = nullptr;
        rc = xbla_copy(ctx, t.orbit, dc_base, &cc, &tb, xbla_find(c, dc_fine));
        if (rc != MBK_OK) return rc;
        rc = xbla_copy(ctx, t.orbit, dc_fine, &cc, &tf, tb);
        if (rc != MBK_OK) return rc;
        fill_xbla_table(fine->wide, cc, tf);
        return MBK_OK;
    }
    const double dc_base = deep_dcmax(&b.deep), dc_fine = deep_dcmax(&f.deep);
    const mbk_ctx::BlaSlot *tb = nullptr, *tf = nullptr;
    rc = bla_copy(ctx, t.orbit, dc_base, &cc, &tb, bla_find(c, dc_fine));
    if (rc != MBK_OK) return rc;
    rc = bla_copy(ctx, t.orbit, dc_fine, &cc, &tf, tb);
    if (rc != MBK_OK) return rc;
    fill_bla_table(fine->deep, cc, tf);
    return MBK_OK;
}

// The waves per SIMD a refine grid asks for: what every instantiation of the kind's kernel holds at once by its registers
// (profiles/refine_walk/README.md has the compiler's table).
static const uint32_t kPlainRefineWaves = 6u;   // 43 .. 77 VGPRs: 6 or 7
static const uint32_t kDeepRefineWaves = 5u;    // 73 .. 85 VGPRs: 5 or 6
static const uint32_t kWideRefineWaves = 5u;    // 65 .. 81 VGPRs: 5 to 7

// What the walk of a refine kernel takes over from the band's classify launch.  d_words: the list's length and the cursor.
static mbk::AdaptiveWalkArgs refine_walk_args(const mbk::AdaptiveClassifyArgs &a, uint32_t *d_words)
{
    mbk::AdaptiveWalkArgs w;
    std::memset(&w, 0, sizeof(w));
    w.nc = a.nc;
    w.list = a.list;
    w.len = d_words;
    w.cursor = d_words + 1;
    w.out = a.out;
    w.out_pitch = a.out_pitch;
    w.stats = a.stats;
    w.pal = a.pal;
    return w;
}

// The grid of a refine kernel on an nc x nr band: `waves` waves per SIMD -- one 256-thread workgroup per CU each --, and no
// more workgroups than groups the fullest list can hold.
static dim3 refine_grid(const mbk_ctx *ctx, uint32_t s, uint32_t nc, uint32_t nr, uint32_t waves)
{
    const uint32_t cus = (uint32_t)std::max(ctx->prop.multiProcessorCount, 1);
    const uint32_t per_group = 64u / (s * s);
    const uint64_t groups = ((uint64_t)nc * nr + per_group - 1u) / per_group;
    return dim3((uint32_t)std::min<uint64_t>((groups + 3u) / 4u, (uint64_t)cus * waves));
}

// The refine step of a plain view's band: the fine samples of the listed pixels on the hand-scheduled loops (mbk_adaptive.h).
// (x0, y0, nc, nr): the band in the W x H view; a: the band's classify launch.
static int launch_plain_refine(mbk_ctx *ctx, const Target &t, uint32_t s, uint32_t x0, uint32_t y0, uint32_t nc, uint32_t nr, uint32_t mrd,
                               bool per_step, const mbk::AdaptiveClassifyArgs &a, uint32_t *d_words, hipStream_t stream)
{
    mbk::AdaptiveRefineArgs f;
    std::memset(&f, 0, sizeof(f));
    f.w = refine_walk_args(a, d_words);
    f.re = make_axis(t.view.start_r, t.view.range_r, t.g.width * s);
    f.im = make_axis(t.view.start_i, t.view.range_i, t.g.height * s);
    f.px0 = x0;
    f.py0 = y0;
    f.mrd = (int32_t)mrd;
    f.exact_steps = ctx->opt[MBK_OPT_EXACT_STEPS];
    f.cyc_window = ctx->opt[MBK_OPT_CYCLE_WINDOW];
    const dim3 grid = refine_grid(ctx, s, nc, nr, kPlainRefineWaves);
    if (per_step) mbk::launch_adaptive_refine<mbk::AdaptiveRefine<0>>(s, grid, stream, f);
    else mbk::launch_adaptive_refine<mbk::AdaptiveRefine<8>>(s, grid, stream, f);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// The refine step of a deep view's band: the fine samples by perturbation (mbk_deep_adaptive.h), with the skips of `fine` where
// it holds a table.
static int launch_deep_refine(mbk_ctx *ctx, const Target &t, uint32_t s, uint32_t x0, uint32_t y0, uint32_t nc, uint32_t nr, uint32_t mrd,
                              const mbk::DeepBlaArgs &fine, const mbk::AdaptiveClassifyArgs &a, uint32_t *d_words, hipStream_t stream)
{
    mbk_ctx::DeepCopy *c = nullptr;
    int rc = deep_copy(ctx, t.orbit, &c);
    if (rc != MBK_OK) return rc;
    const Target samples = target_samples(t, s, x0, y0, nc, nr);
    mbk::DeepAdaptiveRefineArgs f;
    std::memset(&f, 0, sizeof(f));
    f.w = refine_walk_args(a, d_words);
    f.b = fine;
    fill_deep_args(f.b.v, c->d, t.orbit, &samples.deep, mrd);
    const dim3 grid = refine_grid(ctx, s, nc, nr, kDeepRefineWaves);
    if (fine.rc) mbk::launch_adaptive_refine<mbk::DeepAdaptiveRefine<true>>(s, grid, stream, f);
    else mbk::launch_adaptive_refine<mbk::DeepAdaptiveRefine<false>>(s, grid, stream, f);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// The refine step of an extended-range deep view's band: launch_deep_refine's twin in the wide number system
// (mbk_deep_wide_adaptive.h), on the wide orbit table, with the skips of `fine` where it holds a table.
static int launch_deep_wide_refine(mbk_ctx *ctx, const Target &t, uint32_t s, uint32_t x0, uint32_t y0, uint32_t nc, uint32_t nr, uint32_t mrd,
                                   const mbk::DeepWideBlaArgs &fine, const mbk::AdaptiveClassifyArgs &a, uint32_t *d_words, hipStream_t stream)
{
    const mbk::WideEntry *d_orbit = nullptr;
    int rc = wide_copy(ctx, t.orbit, &d_orbit);
    if (rc != MBK_OK) return rc;
    const Target samples = target_samples(t, s, x0, y0, nc, nr);
    mbk::DeepWideAdaptiveRefineArgs f;
    std::memset(&f, 0, sizeof(f));
    f.w = refine_walk_args(a, d_words);
    f.b = fine;
    fill_deep_wide_args(f.b.v, d_orbit, t.orbit, &samples.wide, mrd);
    const dim3 grid = refine_grid(ctx, s, nc, nr, kWideRefineWaves);
    if (fine.ke) mbk::launch_adaptive_refine<mbk::DeepWideAdaptiveRefine<true>>(s, grid, stream, f);
    else mbk::launch_adaptive_refine<mbk::DeepWideAdaptiveRefine<false>>(s, grid, stream, f);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// A checked adaptive render (adaptive_check) onto the device image d_out (ncols x nrows words) and, if not NULL, the device
// mask d_mask (ncols x nrows bytes), on `stream`.  stat: the slot whose reduction scratch the classify and refine kernels add
// their samples' statistics to and whose ev_k1 marks the last kernel (_compute), or NULL.  fine: adaptive_tables' (deep views).
static int adaptive_run(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                        uint32_t threshold, uint32_t *d_out, uint8_t *d_mask, hipStream_t stream, Slot *stat,
                        const AdaptiveFine *fine = nullptr)
{
    const uint32_t s = spec->supersample;
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    rc = stream_palette(ctx, sc, stream, spec->palette, spec->palette_len);
    if (rc != MBK_OK) return rc;

    const BandPlan plan = adaptive_band_plan(t.g.ncols, t.g.nrows, spec->max_band_rows);
    const size_t cap_halo = ((size_t)plan.tile_cols + 2u) * ((size_t)plan.band_rows + 2u);
    // layout: nu | counts (the halo's base samples, as a smooth render's) | list | length, cursor
    const size_t off_counts = round_up_256(cap_halo * 8u);
    const size_t off_list = off_counts + round_up_256(cap_halo * 4u);
    const size_t off_words = off_list + round_up_256(plan.cap_px() * 4u);
    const size_t need = off_words + 256u;
    rc = grow(ctx, sc->d_render, sc->render_cap, need, need);
    if (rc != MBK_OK) return rc;
    uint8_t *base = (uint8_t *)sc->d_render;
    const Outputs samples = {(int32_t *)(base + off_counts), nullptr, (double *)base, false, nullptr, false};
    uint32_t *d_list = (uint32_t *)(base + off_list), *d_words = (uint32_t *)(base + off_words);
    const uint32_t *d_palette = sc->d_palette;   // (sc may move when a launch below adds a stream's scratch: not used past here)

    const size_t lds = (size_t)spec->palette_len * sizeof(uint32_t);
    const size_t tile_lds = mbk::kAdaptiveCells * sizeof(uint32_t);   // (the classify kernel's own, beside the palette)
    const bool use_lds = spec->palette_len <= mbk::kRenderLdsEntries && lds + tile_lds <= ctx->prop.sharedMemPerBlock;
    const uint32_t cus = (uint32_t)std::max(ctx->prop.multiProcessorCount, 1);
    const uint32_t wg_per_cu = use_lds ? (uint32_t)std::min<size_t>(8u, std::max<size_t>(1u, (160u << 10) / (lds + tile_lds))) : 8u;
    const bool per_step = (flags & MBK_KERNEL_MASK) == MBK_KERNEL_ASM;
    ReduceSlot *d_red = stat ? stat->d_red : nullptr;

    rc = for_each_band(ctx, plan, nullptr, 1u, mrd, stream, nullptr, [&](uint32_t r, uint32_t c, uint32_t nr, uint32_t nc, bool is_last) -> int {
        // 1. the base samples of the band's halo: grown by one pixel, clamped to the VIEW
        const uint32_t x0 = t.g.col0 + c, y0 = t.g.row0 + r;
        const uint32_t ox = x0 > 0u ? 1u : 0u, oy = y0 > 0u ? 1u : 0u;
        const uint32_t hc = ox + nc + (x0 + nc < t.g.width ? 1u : 0u), hr = oy + nr + (y0 + nr < t.g.height ? 1u : 0u);
        int rc = target_launch(ctx, target_samples(t, 1u, x0 - ox, y0 - oy, hc, hr), mrd, flags, samples, stream);
        if (rc != MBK_OK) return rc;
        rc = clear_words(ctx, d_words, 2u, stream);
        if (rc != MBK_OK) return rc;
        // 2. classify: base image, mask, list
        mbk::AdaptiveClassifyArgs a;
        std::memset(&a, 0, sizeof(a));
        a.counts = samples.counts;
        a.smooth = samples.values;
        a.hc = hc;
        a.hr = hr;
        a.ox = ox;
        a.oy = oy;
        a.nc = nc;
        a.nr = nr;
        a.tiles_x = (nc + mbk::kAdaptiveTileX - 1u) / mbk::kAdaptiveTileX;
        a.threshold = threshold;
        a.mrd = mrd;
        a.lds_palette = use_lds ? 1u : 0u;
        a.out = d_out + (size_t)r * t.g.ncols + c;
        a.mask = d_mask ? d_mask + (size_t)r * t.g.ncols + c : nullptr;
        a.out_pitch = t.g.ncols;
        a.list = d_list;
        a.len = d_words;
        a.stats = d_red;
        a.pal = render_palette(spec, d_palette);
        const uint64_t tiles = (uint64_t)a.tiles_x * ((nr + mbk::kAdaptiveTileY - 1u) / mbk::kAdaptiveTileY);
        hipLaunchKernelGGL(mbk::adaptive_classify_kernel, dim3((uint32_t)std::min<uint64_t>(tiles, (uint64_t)cus * wg_per_cu)), dim3(256),
                           use_lds ? lds : 0u, stream, a);
        MBK_HIP(ctx, hipGetLastError());
        // 3. refine: the fine samples of the listed pixels (at s = 1 a refined pixel is its base pixel: nothing to do), by the
        // kernel of the kind
        if (s > 1u && threshold < 256u) {
            if (t.kind == Target::kDeep) rc = launch_deep_refine(ctx, t, s, x0, y0, nc, nr, mrd, fine->deep, a, d_words, stream);
            else if (t.kind == Target::kWide) rc = launch_deep_wide_refine(ctx, t, s, x0, y0, nc, nr, mrd, fine->wide, a, d_words, stream);
            else rc = launch_plain_refine(ctx, t, s, x0, y0, nc, nr, mrd, per_step, a, d_words, stream);
            if (rc != MBK_OK) return rc;
        }
        if (stat && is_last) MBK_HIP(ctx, hipEventRecord(stat->ev_k1, stream));
        return MBK_OK;
    });
    if (rc != MBK_OK || !stat) return rc;
    // the kernels have added everything up: only the copy of the partial results is left
    return launch_reduce(ctx, stat->d_red, stat->h_red, nullptr, nullptr, 0u, mrd, stream, false);
}

// The two forms of an adaptive render on a target: device pointers on a stream, host pointers synchronously on slot 0.
static int adaptive_launch(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                           uint32_t threshold, uint8_t *d_rgba, uint8_t *d_mask, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = adaptive_check(ctx, t, mrd, flags, spec, threshold, d_rgba);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    AdaptiveFine fine;
    rc = adaptive_tables(ctx, t, flags, spec->supersample, threshold, &fine);
    if (rc != MBK_OK) return rc;
    return adaptive_run(ctx, t, mrd, flags, spec, threshold, (uint32_t *)d_rgba, d_mask, (hipStream_t)hip_stream, nullptr, &fine);
}

static int adaptive_compute(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                            uint32_t threshold, uint8_t *h_rgba, uint8_t *h_mask, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = adaptive_check(ctx, t, mrd, flags, spec, threshold, h_rgba);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    AdaptiveFine fine;
    rc = adaptive_tables(ctx, t, flags, spec->supersample, threshold, &fine);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    const size_t px = (size_t)t.g.ncols * t.g.nrows;
    auto enqueue = [&]() -> int {
        // the ctx' device image, with the mask behind it: px words and px bytes
        const size_t words = px + (px + 3u) / 4u;
        int rc = grow(ctx, ctx->d_rgba, ctx->rgba_cap_px, words, words * sizeof(uint32_t));
        if (rc != MBK_OK) return rc;
        uint8_t *d_mask = h_mask ? (uint8_t *)(ctx->d_rgba + px) : nullptr;
        MBK_HIP(ctx, hipMemsetAsync(sl.d_red, 0, sizeof(ReduceSlot) * mbk::kReduceSlots, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
        rc = adaptive_run(ctx, t, mrd, flags, spec, threshold, ctx->d_rgba, d_mask, sl.stream, &sl, &fine);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_rgba, ctx->d_rgba, px * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
        if (h_mask) MBK_HIP(ctx, hipMemcpyAsync(h_mask, d_mask, px, hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    return sync_end(ctx, enqueue(), stats, false);
}

int mbk_view_render_adaptive_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                    uint32_t threshold, uint8_t *d_rgba, uint8_t *d_mask, void *hip_stream)
{
    return adaptive_launch(ctx, view_target(view), mrd, flags, spec, threshold, d_rgba, d_mask, hip_stream);
}

int mbk_view_render_adaptive_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                     uint32_t threshold, uint8_t *h_rgba, uint8_t *h_mask, mbk_stats *stats)
{
    return adaptive_compute(ctx, view_target(view), mrd, flags, spec, threshold, h_rgba, h_mask, stats);
}

int mbk_deep_view_render_adaptive_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                         uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *d_rgba,
                                         uint8_t *d_mask, void *hip_stream)
{
    return adaptive_launch(ctx, deep_target(orbit, view), mrd, flags, spec, threshold, d_rgba, d_mask, hip_stream);
}

int mbk_deep_view_render_adaptive_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *h_rgba,
                                          uint8_t *h_mask, mbk_stats *stats)
{
    return adaptive_compute(ctx, deep_target(orbit, view), mrd, flags, spec, threshold, h_rgba, h_mask, stats);
}

int mbk_deep_xview_render_adaptive_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *d_rgba,
                                          uint8_t *d_mask, void *hip_stream)
{
    return adaptive_launch(ctx, wide_target(orbit, view), mrd, flags, spec, threshold, d_rgba, d_mask, hip_stream);
}

int mbk_deep_xview_render_adaptive_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *h_rgba,
                                           uint8_t *h_mask, mbk_stats *stats)
{
    return adaptive_compute(ctx, wide_target(orbit, view), mrd, flags, spec, threshold, h_rgba, h_mask, stats);
}

int mbk_render_adaptive_host(const mbk_render_spec *spec, uint32_t threshold, uint32_t width, uint32_t height,
                             const int32_t *base_counts, const double *base_smooth, const int32_t *fine_counts,
                             const double *fine_smooth, uint8_t *rgba, uint8_t *mask)
{
    int rc = validate_render_spec(nullptr, spec, false);
    if (rc != MBK_OK) return rc;
    if (spec->source != MBK_RENDER_SMOOTH)
        return fail(nullptr, MBK_ERR_INVALID, "adaptive supersampling is implemented for MBK_RENDER_SMOOTH only");
    if (threshold > 256u) return fail(nullptr, MBK_ERR_INVALID, "threshold must lie in [0, 256]");
    if (!rgba) return fail(nullptr, MBK_ERR_INVALID, "output pointer is NULL");
    const uint32_t s = spec->supersample;
    if (width == 0 || height == 0 || (uint64_t)width * s >= (1ull << 31) || (uint64_t)height * s >= (1ull << 31))
        return fail(nullptr, MBK_ERR_INVALID, "width and height must be > 0 and, times supersample, below 2^31");
    if (!base_counts || !base_smooth || !fine_counts || !fine_smooth) return fail(nullptr, MBK_ERR_INVALID, "the sample arrays are NULL");
    std::vector<uint32_t> words(spec->palette_len);
    for (uint32_t k = 0; k < spec->palette_len; ++k) words[k] = pack_rgba(spec->palette + 4u * (size_t)k);
    mbk::render_adaptive_host(render_palette(spec, words.data()), s, threshold, width, height, base_counts, base_smooth, fine_counts,
                              fine_smooth, rgba, mask);
    return MBK_OK;
}

// ---- interior renders (mbk.h "Interior views"): calls of their own on the render machinery above ------------------------

static int validate_interior_spec(mbk_ctx *ctx, const mbk_interior_render_spec *spec)
{
    if (!spec) return fail(ctx, MBK_ERR_INVALID, "render spec is NULL");
    if (!spec->palette) return fail(ctx, MBK_ERR_INVALID, "palette is NULL");
    const uint32_t s = spec->supersample;
    if (s != 1u && s != 2u && s != 3u && s != 4u && s != 8u) return fail(ctx, MBK_ERR_INVALID, "supersample must be 1, 2, 3, 4 or 8");
    if (spec->palette_len < 1u || spec->palette_len > 65536u) return fail(ctx, MBK_ERR_INVALID, "interior renders take a palette of 1 .. 65536 entries");
    if (!(spec->scale > 0.0) || !(spec->scale <= 0x1p80)) return fail(ctx, MBK_ERR_INVALID, "scale must lie in (0, 2^80]");
    return MBK_OK;
}

// The spec as the render machinery reads it (scale, palette, supersampling, banding) and the two colours it has no field for.
static mbk_render_spec interior_render_spec(const mbk_interior_render_spec *spec, InteriorColours *colours)
{
    mbk_render_spec r = {};
    r.source = kRenderSourceInterior;
    r.supersample = spec->supersample;
    r.palette = spec->palette;
    r.palette_len = spec->palette_len;
    r.scale = spec->scale;
    r.max_band_rows = spec->max_band_rows;
    colours->unknown = pack_rgba(spec->unknown);
    colours->outside = pack_rgba(spec->outside);
    return r;
}

// Everything an interior render can refuse, before anything is allocated, enqueued or written.
static int interior_render_check(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_interior_render_spec *spec,
                                 const void *out, Target *t)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = validate_interior_spec(ctx, spec);
    if (rc != MBK_OK) return rc;
    *t = view_target(view);
    const uint32_t s = spec->supersample;
    rc = render_geometry_check(ctx, *t, s, out);
    if (rc != MBK_OK) return rc;
    const Target samples = target_samples(*t, s, t->g.col0, t->g.row0, t->g.ncols, t->g.nrows);
    bool safe = false;
    return interior_check(ctx, &samples.view, mrd, flags, &safe);
}

int mbk_view_interior_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                                    const mbk_interior_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    Target t;
    int rc = interior_render_check(ctx, view, mrd, flags, spec, d_rgba, &t);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    InteriorColours colours;
    const mbk_render_spec r = interior_render_spec(spec, &colours);
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags, &r, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr, nullptr, 0u, &colours);
}

int mbk_view_interior_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                                     const mbk_interior_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    Target t;
    int rc = interior_render_check(ctx, view, mrd, flags, spec, h_rgba, &t);
    if (rc != MBK_OK) return rc;
    InteriorColours colours;
    const mbk_render_spec r = interior_render_spec(spec, &colours);
    return render_compute_checked(ctx, t, mrd, flags, &r, h_rgba, stats, nullptr, 0u, &colours);
}

int mbk_interior_resolve_host(const mbk_interior_render_spec *spec, uint32_t width, uint32_t height, const int32_t *counts,
                              const int32_t *period, const double *de, uint8_t *rgba)
{
    int rc = validate_interior_spec(nullptr, spec);
    if (rc != MBK_OK) return rc;
    if (!rgba) return fail(nullptr, MBK_ERR_INVALID, "output pointer is NULL");
    const uint32_t s = spec->supersample;
    if (width == 0 || height == 0 || (uint64_t)width * s >= (1ull << 31) || (uint64_t)height * s >= (1ull << 31))
        return fail(nullptr, MBK_ERR_INVALID, "width and height must be > 0 and, times supersample, below 2^31");
    if (!counts || !period || !de) return fail(nullptr, MBK_ERR_INVALID, "the sample arrays are NULL");
    InteriorColours colours;
    const mbk_render_spec r = interior_render_spec(spec, &colours);
    std::vector<uint32_t> words(spec->palette_len);
    for (uint32_t k = 0; k < spec->palette_len; ++k) words[k] = pack_rgba(spec->palette + 4u * (size_t)k);
    mbk::RenderPalette pal = render_palette(&r, words.data());
    pal.unknown = colours.unknown;
    pal.outside = colours.outside;
    mbk::render_resolve_host(pal, true, s, width, height, counts, nullptr, de, rgba, mbk::kRuleInterior, period);
    return MBK_OK;
}

// ---- relief renders (mbk.h "Relief shading"): calls of their own on the render machinery above -------------------------

// The spec as the render machinery reads it: an MBK_RENDER_SMOOTH render of the same palette; and the light.
static mbk_render_spec relief_render_spec(const mbk_relief_spec *spec, ReliefLight *light)
{
    mbk_render_spec r = {};
    r.source = MBK_RENDER_SMOOTH;
    r.supersample = spec->supersample;
    r.palette = spec->palette;
    r.palette_len = spec->palette_len;
    std::memcpy(r.inside, spec->inside, sizeof(r.inside));
    r.scale = spec->scale;
    r.offset = spec->offset;
    r.max_band_rows = spec->max_band_rows;
    light->x = spec->light_x;
    light->y = spec->light_y;
    light->height = spec->height;
    return r;
}

// What a relief spec adds to an MBK_RENDER_SMOOTH one (validate_render_spec checks the rest): the light and the height.
static int validate_relief_light(mbk_ctx *ctx, const mbk_relief_spec *spec)
{
    if (!(std::fabs(spec->light_x) <= 1.0) || !(std::fabs(spec->light_y) <= 1.0))
        return fail(ctx, MBK_ERR_INVALID, "light_x and light_y must lie in [-1, 1]");
    if (!(spec->height >= 0.0) || !(spec->height <= 0x1p10)) return fail(ctx, MBK_ERR_INVALID, "height must lie in [0, 2^10]");
    return MBK_OK;
}

// Everything a relief render can refuse, before anything is allocated, enqueued or written: what an MBK_RENDER_SMOOTH render
// of the view refuses, MBK_PRECISION_F32 among it, and a light or a height out of range.
static int relief_render_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_relief_spec *spec, const void *out,
                               mbk_render_spec *r, ReliefLight *light)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!spec) return fail(ctx, MBK_ERR_INVALID, "render spec is NULL");
    *r = relief_render_spec(spec, light);
    int rc = render_check(ctx, t, mrd, flags, r, out);
    if (rc != MBK_OK) return rc;
    return validate_relief_light(ctx, spec);
}

int mbk_view_relief_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_relief_spec *spec,
                                  uint8_t *d_rgba, void *hip_stream)
{
    const Target t = view_target(view);
    mbk_render_spec r;
    ReliefLight light;
    int rc = relief_render_check(ctx, t, mrd, flags, spec, d_rgba, &r, &light);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags, &r, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr, nullptr, 0u, nullptr, &light);
}

int mbk_view_relief_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_relief_spec *spec,
                                   uint8_t *h_rgba, mbk_stats *stats)
{
    const Target t = view_target(view);
    mbk_render_spec r;
    ReliefLight light;
    int rc = relief_render_check(ctx, t, mrd, flags, spec, h_rgba, &r, &light);
    if (rc != MBK_OK) return rc;
    return render_compute_checked(ctx, t, mrd, flags, &r, h_rgba, stats, nullptr, 0u, nullptr, &light);
}

int mbk_relief_resolve_host(const mbk_relief_spec *spec, uint32_t width, uint32_t height, const int32_t *counts, const double *smooth,
                            const double *normals, uint8_t *rgba)
{
    if (!spec) return fail(nullptr, MBK_ERR_INVALID, "render spec is NULL");
    ReliefLight light;
    const mbk_render_spec r = relief_render_spec(spec, &light);
    int rc = validate_render_spec(nullptr, &r);
    if (rc == MBK_OK) rc = validate_relief_light(nullptr, spec);
    if (rc != MBK_OK) return rc;
    if (!rgba) return fail(nullptr, MBK_ERR_INVALID, "output pointer is NULL");
    const uint32_t s = spec->supersample;
    if (width == 0 || height == 0 || (uint64_t)width * s >= (1ull << 31) || (uint64_t)height * s >= (1ull << 31))
        return fail(nullptr, MBK_ERR_INVALID, "width and height must be > 0 and, times supersample, below 2^31");
    if (!counts || !smooth || !normals) return fail(nullptr, MBK_ERR_INVALID, "the sample arrays are NULL");
    std::vector<uint32_t> words(spec->palette_len);
    for (uint32_t k = 0; k < spec->palette_len; ++k) words[k] = pack_rgba(spec->palette + 4u * (size_t)k);
    mbk::RenderPalette pal = render_palette(&r, words.data());
    pal.light_x = light.x;
    pal.light_y = light.y;
    pal.height = light.height;
    mbk::render_resolve_host(pal, true, s, width, height, counts, nullptr, smooth, rgba, mbk::kRuleRelief, nullptr, normals);
    return MBK_OK;
}

// ---- stripe renders (mbk.h "Stripe-average colouring"): calls of their own on the render machinery above ---------------

// The spec as the render machinery reads it: an MBK_RENDER_SMOOTH render of the same palette; and the stripe parameters.
static mbk_render_spec stripe_render_spec(const mbk_stripe_spec *spec, StripeShade *shade)
{
    mbk_render_spec r = {};
    r.source = MBK_RENDER_SMOOTH;
    r.supersample = spec->supersample;
    r.palette = spec->palette;
    r.palette_len = spec->palette_len;
    std::memcpy(r.inside, spec->inside, sizeof(r.inside));
    r.scale = spec->scale;
    r.offset = spec->offset;
    r.max_band_rows = spec->max_band_rows;
    shade->density = spec->density;
    shade->skip = spec->skip;
    shade->lo = spec->lo;
    shade->gain = spec->gain;
    return r;
}

// What a stripe spec adds to an MBK_RENDER_SMOOTH one (validate_render_spec checks the rest).
static int validate_stripe_shade(mbk_ctx *ctx, const mbk_stripe_spec *spec)
{
    if (spec->density < 1u || spec->density > mbk::kStripeDensityMax) return fail(ctx, MBK_ERR_INVALID, "density must lie in 1 .. 16");
    if (spec->skip > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "skip must lie in 0 .. 2^31 - 1");
    if (!(spec->lo >= 0.0) || !(spec->lo <= 1.0)) return fail(ctx, MBK_ERR_INVALID, "lo must lie in [0, 1]");
    if (!(spec->gain >= 0.0) || !(spec->gain <= 0x1p10)) return fail(ctx, MBK_ERR_INVALID, "gain must lie in [0, 2^10]");
    return MBK_OK;
}

// Everything a stripe render can refuse, before anything is allocated, enqueued or written: what an MBK_RENDER_SMOOTH render
// of the view refuses, MBK_PRECISION_F32 among it, and stripe parameters out of range.
static int stripe_render_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_stripe_spec *spec, const void *out,
                               mbk_render_spec *r, StripeShade *shade)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!spec) return fail(ctx, MBK_ERR_INVALID, "render spec is NULL");
    *r = stripe_render_spec(spec, shade);
    int rc = render_check(ctx, t, mrd, flags, r, out);
    if (rc != MBK_OK) return rc;
    return validate_stripe_shade(ctx, spec);
}

int mbk_view_stripe_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_stripe_spec *spec,
                                  uint8_t *d_rgba, void *hip_stream)
{
    const Target t = view_target(view);
    mbk_render_spec r;
    StripeShade shade;
    int rc = stripe_render_check(ctx, t, mrd, flags, spec, d_rgba, &r, &shade);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags, &r, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr, nullptr, 0u, nullptr, nullptr, &shade);
}

int mbk_view_stripe_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_stripe_spec *spec,
                                   uint8_t *h_rgba, mbk_stats *stats)
{
    const Target t = view_target(view);
    mbk_render_spec r;
    StripeShade shade;
    int rc = stripe_render_check(ctx, t, mrd, flags, spec, h_rgba, &r, &shade);
    if (rc != MBK_OK) return rc;
    return render_compute_checked(ctx, t, mrd, flags, &r, h_rgba, stats, nullptr, 0u, nullptr, nullptr, &shade);
}

int mbk_stripe_resolve_host(const mbk_stripe_spec *spec, uint32_t width, uint32_t height, const int32_t *counts, const double *smooth,
                            const double *stripe, uint8_t *rgba)
{
    if (!spec) return fail(nullptr, MBK_ERR_INVALID, "render spec is NULL");
    StripeShade shade;
    const mbk_render_spec r = stripe_render_spec(spec, &shade);
    int rc = validate_render_spec(nullptr, &r);
    if (rc == MBK_OK) rc = validate_stripe_shade(nullptr, spec);
    if (rc != MBK_OK) return rc;
    if (!rgba) return fail(nullptr, MBK_ERR_INVALID, "output pointer is NULL");
    const uint32_t s = spec->supersample;
    if (width == 0 || height == 0 || (uint64_t)width * s >= (1ull << 31) || (uint64_t)height * s >= (1ull << 31))
        return fail(nullptr, MBK_ERR_INVALID, "width and height must be > 0 and, times supersample, below 2^31");
    if (!counts || !smooth || !stripe) return fail(nullptr, MBK_ERR_INVALID, "the sample arrays are NULL");
    std::vector<uint32_t> words(spec->palette_len);
    for (uint32_t k = 0; k < spec->palette_len; ++k) words[k] = pack_rgba(spec->palette + 4u * (size_t)k);
    mbk::RenderPalette pal = render_palette(&r, words.data());
    pal.stripe_lo = shade.lo;
    pal.stripe_gain = shade.gain;
    mbk::render_resolve_host(pal, true, s, width, height, counts, nullptr, smooth, rgba, mbk::kRuleStripe, nullptr, nullptr, stripe);
    return MBK_OK;
}

// ---- relief shading for deep views (mbk_deep_relief.h; mbk.h "Relief shading for deep views"): the value calls on the
// scaffold of the value calls, the renders on the relief render path above ---------------------------------------------------

// Everything a deep normal call can refuse, before anything is allocated, enqueued or written: the NULL pointers, every flag but
// MBK_DEEP_BLA, then the rules of the count launch under the same flag (the table's indices must fit).
static int deep_normal_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const void *normal)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!normal) return fail(ctx, MBK_ERR_INVALID, "NULL normal pointer");
    if (flags & ~(uint32_t)MBK_DEEP_BLA) return fail(ctx, MBK_ERR_INVALID, "deep normals take MBK_DEEP_BLA only (no kernel selection, no fp32)");
    return target_check(ctx, t, mrd, flags);
}

int mbk_deep_view_launch_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                                int32_t *d_counts, double *d_normal, double *d_smooth, double *d_rel, void *hip_stream)
{
    const Target t = deep_target(orbit, view);
    int rc = deep_normal_check(ctx, t, mrd, flags, d_normal);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_normal & 7u) return fail(ctx, MBK_ERR_INVALID, "d_normal must be 8-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return target_launch(ctx, t, mrd, flags, Outputs{d_counts, nullptr, d_smooth, false, nullptr, false, d_normal, d_rel}, (hipStream_t)hip_stream);
}

int mbk_deep_view_compute_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                                 int32_t *h_counts, double *h_normal, double *h_smooth, double *h_rel, mbk_stats *stats)
{
    const Target t = deep_target(orbit, view);
    int rc = deep_normal_check(ctx, t, mrd, flags, h_normal);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    // the device values: 2 px binary64 (the normals), then px (nu), then px (rel)
    const size_t px = (size_t)t.g.ncols * t.g.nrows;
    return compute_values(ctx, px, mrd, h_counts, h_normal, stats,
                          [&](int32_t *d_counts, double *d_normal, hipStream_t stream) {
                              return target_launch(ctx, t, mrd, flags,
                                                   Outputs{d_counts, nullptr, h_smooth ? d_normal + 2u * px : nullptr, false, nullptr, false,
                                                           d_normal, h_rel ? d_normal + 3u * px : nullptr},
                                                   stream);
                          },
                          false, nullptr, 2u, h_smooth, h_rel);
}

int mbk_deep_view_relief_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                                       const mbk_relief_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    const Target t = deep_target(orbit, view);
    mbk_render_spec r;
    ReliefLight light;
    int rc = relief_render_check(ctx, t, mrd, flags, spec, d_rgba, &r, &light);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags, &r, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr, nullptr, 0u, nullptr, &light);
}

int mbk_deep_view_relief_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                                        const mbk_relief_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    const Target t = deep_target(orbit, view);
    mbk_render_spec r;
    ReliefLight light;
    int rc = relief_render_check(ctx, t, mrd, flags, spec, h_rgba, &r, &light);
    if (rc != MBK_OK) return rc;
    return render_compute_checked(ctx, t, mrd, flags, &r, h_rgba, stats, nullptr, 0u, nullptr, &light);
}

// host twin (the loop of mbk_deep_distance_bla.h's, the epilogue of mbk_deep_relief.h): no ctx, no device.  flags 0: no table,
// the plain rule
int mbk_deep_normal_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd, uint32_t flags,
                         int32_t *count, int32_t *extra, double *zp_r, double *zp_i, double *D_r, double *D_i, int32_t *e, double normal[2],
                         double *nu, uint64_t *steps_executed)
{
    if (!count || !extra || !zp_r || !zp_i || !D_r || !D_i || !e || !normal || !nu || !steps_executed)
        return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    if (flags & ~(uint32_t)MBK_DEEP_BLA) return fail(nullptr, MBK_ERR_INVALID, "deep normals take MBK_DEEP_BLA only (no kernel selection, no fp32)");
    mbk::BlaTable t;
    int rc = (flags & MBK_DEEP_BLA) ? bla_host_table(orbit, view, &t) : validate_deep(nullptr, orbit, view, 0u, 0u);
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(nullptr, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    double mag = 0.0, escaped = 0.0;   // (the final mag is the distance twin's to report)
    mbk::deep_distance_bla_host(orbit->o.table, orbit->o.length, t, dc.r, dc.i, (int64_t)mrd, count, extra, &mag, D_r, D_i, e, steps_executed,
                                zp_r, zp_i, &escaped);
    mbk::normal_value(*zp_r, *zp_i, *D_r, *D_i, *count, normal);
    *nu = mbk::smooth_value(*count, escaped);
    return MBK_OK;
}

// ---- relief shading for extended-range deep views (mbk_deep_wide_relief.h; mbk.h, the section of that name): the calls of the
// deep views on a Target of kind kWide ------------------------------------------------------------------------------------------

// What the wide relief calls refuse of their flags: MBK_DEEP_BLA in validate_deep_wide's words, every flag but MBK_DEEP_XBLA
static int wide_normal_flags_check(mbk_ctx *ctx, uint32_t flags)
{
    if (flags & MBK_DEEP_BLA) return fail(ctx, MBK_ERR_INVALID, kNoWideBla);
    if (flags & ~(uint32_t)MBK_DEEP_XBLA)
        return fail(ctx, MBK_ERR_INVALID, "extended-range deep normals take MBK_DEEP_XBLA only (no kernel selection, no fp32)");
    return MBK_OK;
}

// Everything a wide normal call can refuse, before anything is allocated, enqueued or written: the NULL pointers, the flags,
// then the rules of the count launch under the same flag (the table's indices must fit).
static int wide_normal_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const void *normal)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!normal) return fail(ctx, MBK_ERR_INVALID, "NULL normal pointer");
    int rc = wide_normal_flags_check(ctx, flags);
    if (rc != MBK_OK) return rc;
    return target_check(ctx, t, mrd, flags);
}

// relief_render_check behind the flag rules of the wide normal calls
static int wide_relief_render_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const mbk_relief_spec *spec, const void *out,
                                    mbk_render_spec *r, ReliefLight *light)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = wide_normal_flags_check(ctx, flags);
    if (rc != MBK_OK) return rc;
    return relief_render_check(ctx, t, mrd, flags, spec, out, r, light);
}

int mbk_deep_xview_launch_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                                 int32_t *d_counts, double *d_normal, double *d_smooth, double *d_rel, void *hip_stream)
{
    const Target t = wide_target(orbit, view);
    int rc = wide_normal_check(ctx, t, mrd, flags, d_normal);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_normal & 7u) return fail(ctx, MBK_ERR_INVALID, "d_normal must be 8-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return target_launch(ctx, t, mrd, flags, Outputs{d_counts, nullptr, d_smooth, false, nullptr, false, d_normal, d_rel}, (hipStream_t)hip_stream);
}

int mbk_deep_xview_compute_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                                  int32_t *h_counts, double *h_normal, double *h_smooth, double *h_rel, mbk_stats *stats)
{
    const Target t = wide_target(orbit, view);
    int rc = wide_normal_check(ctx, t, mrd, flags, h_normal);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    // the device values: 2 px binary64 (the normals), then px (nu), then px (rel)
    const size_t px = (size_t)t.g.ncols * t.g.nrows;
    return compute_values(ctx, px, mrd, h_counts, h_normal, stats,
                          [&](int32_t *d_counts, double *d_normal, hipStream_t stream) {
                              return target_launch(ctx, t, mrd, flags,
                                                   Outputs{d_counts, nullptr, h_smooth ? d_normal + 2u * px : nullptr, false, nullptr, false,
                                                           d_normal, h_rel ? d_normal + 3u * px : nullptr},
                                                   stream);
                          },
                          false, nullptr, 2u, h_smooth, h_rel);
}

int mbk_deep_xview_relief_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                                        const mbk_relief_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    const Target t = wide_target(orbit, view);
    mbk_render_spec r;
    ReliefLight light;
    int rc = wide_relief_render_check(ctx, t, mrd, flags, spec, d_rgba, &r, &light);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags, &r, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr, nullptr, 0u, nullptr, &light);
}

int mbk_deep_xview_relief_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                                         const mbk_relief_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    const Target t = wide_target(orbit, view);
    mbk_render_spec r;
    ReliefLight light;
    int rc = wide_relief_render_check(ctx, t, mrd, flags, spec, h_rgba, &r, &light);
    if (rc != MBK_OK) return rc;
    return render_compute_checked(ctx, t, mrd, flags, &r, h_rgba, stats, nullptr, 0u, nullptr, &light);
}

// host twin (the loop of mbk_deep_wide_distance_bla.h's, the epilogue of mbk_deep_wide_relief.h): no ctx, no device.  flags 0:
// no table, the plain rule
int mbk_deep_xview_normal_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                               uint32_t flags, int32_t *count, int32_t *extra, double *zp_r, double *zp_i, int32_t *zp_t, double *D_r,
                               double *D_i, int32_t *e, double normal[2], double *nu, uint64_t *steps_executed)
{
    if (!count || !extra || !zp_r || !zp_i || !zp_t || !D_r || !D_i || !e || !normal || !nu || !steps_executed)
        return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = wide_normal_flags_check(nullptr, flags);
    if (rc != MBK_OK) return rc;
    mbk::WideBlaTable t;
    rc = (flags & MBK_DEEP_XBLA) ? xbla_host_table(orbit, view, &t) : validate_deep_wide(nullptr, orbit, view, 0u, 0u);
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(nullptr, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    double mag = 0.0, escaped = 0.0;   // (the final mag is the distance twin's to report)
    mbk::wide_distance_bla_host(orbit->o.wide, orbit->o.length, t, dc.r, dc.i, view->exp2, (int64_t)mrd, count, extra, &mag, D_r, D_i, e,
                                steps_executed, zp_r, zp_i, zp_t, &escaped);
    mbk::normal_value(*zp_r, *zp_i, *D_r, *D_i, *count, normal);
    *nu = mbk::smooth_value(*count, escaped);
    return MBK_OK;
}

// ---- the distance calls (mbk.h, the six "Distance estimates ..." sections; DESIGN.md "One target, four kinds of view"): the
// value calls of six rules on one scaffold, and the renders of the four rules that have calls of their own on another (plain
// views and deep views without skips render through mbk_view_render_* / mbk_deep_view_render_*, which refuse the other four) ---

// A rule.  check: everything its calls can refuse beyond the NULL pointers, before anything is allocated, enqueued or written,
// on the target of a value call or on the samples of a render.  launch_flags: what the launch takes beyond the caller's flags
// (which the check has passed): the skips that the rule's name selects.  source, other_source: the one source the rule's renders
// take and the text that refuses every other; a rule without renders of its own has neither.
struct DistanceRule {
    int (*check)(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags);
    uint32_t launch_flags;
    uint32_t source;
    const char *other_source;
};

static int plain_distance_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    bool safe = false;   // (target_launch derives it again)
    return distance_check(ctx, t.has_view ? &t.view : nullptr, mrd, flags, &safe);
}

// its own flag rule (kernel selection only), then the rules of the count launch
static int julia_distance_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    if (flags & ~(uint32_t)MBK_KERNEL_MASK)
        return fail(ctx, MBK_ERR_INVALID, "Julia distance estimates take kernel selection only (binary64; no MBK_LAZY_UNIFORM, no MBK_DEEP_BLA / MBK_DEEP_XBLA)");
    return target_check(ctx, t, mrd, flags);
}

// The deep rules take no flags, then the rules of the count launch with `skips`: the flag of the count calls that the rule's
// name implies (the table's indices must fit), or none.
static int deep_no_flags_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, uint32_t skips)
{
    if (flags) return fail(ctx, MBK_ERR_INVALID, "deep distance estimates take no flags (no kernel selection, no fp32)");
    return target_check(ctx, t, mrd, skips);
}

static int deep_distance_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    return deep_no_flags_check(ctx, t, mrd, flags, 0u);
}

static int deep_distance_bla_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    if (flags & MBK_DEEP_BLA)
        return fail(ctx, MBK_ERR_INVALID, "the _distance_bla calls take no flags: the name selects the rule (MBK_DEEP_BLA is a flag of the count calls)");
    return deep_no_flags_check(ctx, t, mrd, flags, MBK_DEEP_BLA);
}

// the same for the extended-range rules, which name MBK_DEEP_BLA as the count calls do
static int wide_no_flags_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, uint32_t skips)
{
    if (flags & MBK_DEEP_BLA) return fail(ctx, MBK_ERR_INVALID, kNoWideBla);
    if (flags) return fail(ctx, MBK_ERR_INVALID, "extended-range deep distance estimates take no flags (no kernel selection, no fp32)");
    return target_check(ctx, t, mrd, skips);
}

static int wide_distance_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    if (flags & MBK_DEEP_XBLA)
        return fail(ctx, MBK_ERR_INVALID, "MBK_DEEP_XBLA is not implemented for extended-range deep distance estimates");
    return wide_no_flags_check(ctx, t, mrd, flags, 0u);
}

static int wide_distance_xbla_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags)
{
    if (flags & MBK_DEEP_XBLA)
        return fail(ctx, MBK_ERR_INVALID, "the _distance_xbla calls take no flags: the name selects the rule (MBK_DEEP_XBLA is a flag of the count calls)");
    return wide_no_flags_check(ctx, t, mrd, flags, MBK_DEEP_XBLA);
}

static const DistanceRule kPlainDistance = {plain_distance_check, 0u, 0u, nullptr};
static const DistanceRule kJuliaDistance = {julia_distance_check, 0u, MBK_RENDER_DISTANCE, "Julia distance renders take MBK_RENDER_DISTANCE only"};
static const DistanceRule kDeepDistance = {deep_distance_check, 0u, 0u, nullptr};
static const DistanceRule kDeepDistanceBla = {deep_distance_bla_check, MBK_DEEP_BLA, MBK_RENDER_DISTANCE_REL,
                                              "deep distance renders with bilinear approximation take MBK_RENDER_DISTANCE_REL only"};
static const DistanceRule kWideDistance = {wide_distance_check, 0u, MBK_RENDER_DISTANCE_REL,
                                           "extended-range deep distance renders take MBK_RENDER_DISTANCE_REL only"};
static const DistanceRule kWideDistanceXbla = {wide_distance_xbla_check, MBK_DEEP_XBLA, MBK_RENDER_DISTANCE_REL,
                                               "extended-range deep distance renders with bilinear approximation take MBK_RENDER_DISTANCE_REL only"};

// The two forms of a value call: device pointers on a stream, host pointers synchronously.  The counts pointer may be NULL.
static int distance_values_check(mbk_ctx *ctx, const DistanceRule &rule, const Target &t, uint32_t mrd, uint32_t flags, const void *values)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!values) return fail(ctx, MBK_ERR_INVALID, "NULL value pointer");
    return rule.check(ctx, t, mrd, flags);
}

static int distance_values_launch(mbk_ctx *ctx, const DistanceRule &rule, const Target &t, uint32_t mrd, uint32_t flags, int32_t *d_counts,
                                  double *d_values, void *hip_stream)
{
    int rc = distance_values_check(ctx, rule, t, mrd, flags, d_values);
    if (rc != MBK_OK) return rc;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return target_launch(ctx, t, mrd, flags | rule.launch_flags, Outputs{d_counts, nullptr, d_values, true}, (hipStream_t)hip_stream);
}

static int distance_values_compute(mbk_ctx *ctx, const DistanceRule &rule, const Target &t, uint32_t mrd, uint32_t flags, int32_t *h_counts,
                                   double *h_values, mbk_stats *stats)
{
    int rc = distance_values_check(ctx, rule, t, mrd, flags, h_values);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    return compute_values(ctx, (size_t)t.g.ncols * t.g.nrows, mrd, h_counts, h_values, stats,
                          [&](int32_t *d_counts, double *d_values, hipStream_t stream) {
                              return target_launch(ctx, t, mrd, flags | rule.launch_flags, Outputs{d_counts, nullptr, d_values, true}, stream);
                          });
}

// Everything a render of a rule's own can refuse, before anything is allocated, enqueued or written; then its two forms, on the
// render machinery above.
static int distance_render_check(mbk_ctx *ctx, const DistanceRule &rule, const Target &t, uint32_t mrd, uint32_t flags,
                                 const mbk_render_spec *spec, const void *out)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = validate_render_spec(ctx, spec);
    if (rc != MBK_OK) return rc;
    if (spec->source != rule.source) return fail(ctx, MBK_ERR_INVALID, rule.other_source);
    rc = render_geometry_check(ctx, t, spec->supersample, out);
    if (rc != MBK_OK) return rc;
    return rule.check(ctx, target_samples(t, spec->supersample, t.g.col0, t.g.row0, t.g.ncols, t.g.nrows), mrd, flags);
}

static int distance_render_launch(mbk_ctx *ctx, const DistanceRule &rule, const Target &t, uint32_t mrd, uint32_t flags,
                                  const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    int rc = distance_render_check(ctx, rule, t, mrd, flags, spec, d_rgba);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return render_run(ctx, t, mrd, flags | rule.launch_flags, spec, (uint32_t *)d_rgba, (hipStream_t)hip_stream, nullptr);
}

static int distance_render_compute(mbk_ctx *ctx, const DistanceRule &rule, const Target &t, uint32_t mrd, uint32_t flags,
                                   const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    int rc = distance_render_check(ctx, rule, t, mrd, flags, spec, h_rgba);
    if (rc != MBK_OK) return rc;
    return render_compute_checked(ctx, t, mrd, flags | rule.launch_flags, spec, h_rgba, stats, nullptr, 0u);
}

// The plain pair has one text of its own for its NULL pointers, and its compute form counts the view among them.
int mbk_view_launch_distance(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                             int32_t *d_counts, double *d_distance, void *hip_stream)
{
    if (!ctx || !d_distance) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    return distance_values_launch(ctx, kPlainDistance, view_target(view), mrd, flags, d_counts, d_distance, hip_stream);
}

// (only the kernel selector and MBK_DEEP_XBLA reach the rule: this form serves every other flag, MBK_PRECISION_F32 among them)
int mbk_view_compute_distance(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                              int32_t *h_counts, double *h_distance, mbk_stats *stats)
{
    if (!ctx || !view || !h_distance) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    return distance_values_compute(ctx, kPlainDistance, view_target(view), mrd, flags & (MBK_KERNEL_MASK | MBK_DEEP_XBLA), h_counts, h_distance, stats);
}

int mbk_julia_view_launch_distance(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                   int32_t *d_counts, double *d_distance, void *hip_stream)
{
    return distance_values_launch(ctx, kJuliaDistance, julia_target(view, c_r, c_i), mrd, flags, d_counts, d_distance, hip_stream);
}

int mbk_julia_view_compute_distance(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                    int32_t *h_counts, double *h_distance, mbk_stats *stats)
{
    return distance_values_compute(ctx, kJuliaDistance, julia_target(view, c_r, c_i), mrd, flags, h_counts, h_distance, stats);
}

int mbk_julia_view_distance_render_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                          const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return distance_render_launch(ctx, kJuliaDistance, julia_target(view, c_r, c_i), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_julia_view_distance_render_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                           const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return distance_render_compute(ctx, kJuliaDistance, julia_target(view, c_r, c_i), mrd, flags, spec, h_rgba, stats);
}

int mbk_deep_view_launch_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                  uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream)
{
    return distance_values_launch(ctx, kDeepDistance, deep_target(orbit, view), mrd, flags, d_counts, d_rel, hip_stream);
}

int mbk_deep_view_compute_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                   uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats)
{
    return distance_values_compute(ctx, kDeepDistance, deep_target(orbit, view), mrd, flags, h_counts, h_rel, stats);
}

int mbk_deep_view_launch_distance_bla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                      uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream)
{
    return distance_values_launch(ctx, kDeepDistanceBla, deep_target(orbit, view), mrd, flags, d_counts, d_rel, hip_stream);
}

int mbk_deep_view_compute_distance_bla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                       uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats)
{
    return distance_values_compute(ctx, kDeepDistanceBla, deep_target(orbit, view), mrd, flags, h_counts, h_rel, stats);
}

int mbk_deep_view_distance_bla_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                             uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return distance_render_launch(ctx, kDeepDistanceBla, deep_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_deep_view_distance_bla_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                              uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return distance_render_compute(ctx, kDeepDistanceBla, deep_target(orbit, view), mrd, flags, spec, h_rgba, stats);
}

int mbk_deep_xview_launch_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                   uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream)
{
    return distance_values_launch(ctx, kWideDistance, wide_target(orbit, view), mrd, flags, d_counts, d_rel, hip_stream);
}

int mbk_deep_xview_compute_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                    uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats)
{
    return distance_values_compute(ctx, kWideDistance, wide_target(orbit, view), mrd, flags, h_counts, h_rel, stats);
}

int mbk_deep_xview_distance_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return distance_render_launch(ctx, kWideDistance, wide_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_deep_xview_distance_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return distance_render_compute(ctx, kWideDistance, wide_target(orbit, view), mrd, flags, spec, h_rgba, stats);
}

int mbk_deep_xview_launch_distance_xbla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                        uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream)
{
    return distance_values_launch(ctx, kWideDistanceXbla, wide_target(orbit, view), mrd, flags, d_counts, d_rel, hip_stream);
}

int mbk_deep_xview_compute_distance_xbla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                         uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats)
{
    return distance_values_compute(ctx, kWideDistanceXbla, wide_target(orbit, view), mrd, flags, h_counts, h_rel, stats);
}

int mbk_deep_xview_distance_xbla_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                               uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    return distance_render_launch(ctx, kWideDistanceXbla, wide_target(orbit, view), mrd, flags, spec, d_rgba, hip_stream);
}

int mbk_deep_xview_distance_xbla_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                                uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    return distance_render_compute(ctx, kWideDistanceXbla, wide_target(orbit, view), mrd, flags, spec, h_rgba, stats);
}

// ---- distance estimates for deep views with bilinear approximation (mbk_deep_distance_bla.h; mbk.h, the section of that
// name): the calls stand with the distance calls, above ----------------------------------------------------------------------

// host twins (mbk_deep_distance_bla.h): no ctx, no device
int mbk_deep_distance_bla_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                               int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e, double *rel,
                               uint64_t *steps_executed)
{
    if (!count || !extra || !mag || !D_r || !D_i || !e || !rel || !steps_executed) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::BlaTable t;
    int rc = bla_host_table(orbit, view, &t);
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(nullptr, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::deep_distance_bla_host(orbit->o.table, orbit->o.length, t, dc.r, dc.i, (int64_t)mrd, count, extra, mag, D_r, D_i, e, steps_executed);
    const double r2 = *D_r * *D_r, i2 = *D_i * *D_i;
    *rel = mbk::deep_distance_value(*mag, r2 + i2, *e, view->range_r, *count);
    return MBK_OK;
}

int mbk_deep_distance_bla_skip_host(double A_r, double A_i, double B_r, double B_i, double *D_r, double *D_i, int32_t *e)
{
    if (!D_r || !D_i || !e) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::deep_derivative_skip(A_r, A_i, B_r, B_i, *D_r, *D_i, *e);
    return MBK_OK;
}

// ---- distance estimates for extended-range deep views with bilinear approximation (mbk_deep_wide_distance_bla.h; mbk.h, the
// section of that name): the calls stand with the distance calls, above ------------------------------------------------------

// host twins (mbk_deep_wide_distance_bla.h): no ctx, no device
int mbk_deep_xview_distance_xbla_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                                      int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e, double *rel,
                                      uint64_t *steps_executed)
{
    if (!count || !extra || !mag || !D_r || !D_i || !e || !rel || !steps_executed) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::WideBlaTable t;
    int rc = xbla_host_table(orbit, view, &t);
    if (rc != MBK_OK) return rc;
    if (mrd > orbit->o.mrd) return fail(nullptr, MBK_ERR_INVALID, "mrd exceeds the mrd the reference orbit was computed for");
    const PixelDc dc = pixel_dc(view, col, row);
    if (dc.rc != MBK_OK) return dc.rc;
    mbk::wide_distance_bla_host(orbit->o.wide, orbit->o.length, t, dc.r, dc.i, view->exp2, (int64_t)mrd, count, extra, mag, D_r, D_i, e,
                                steps_executed);
    const double r2 = *D_r * *D_r, i2 = *D_i * *D_i;
    *rel = mbk::wide_distance_value(*mag, r2 + i2, *e, view->range_r, view->exp2, *count);
    return MBK_OK;
}

int mbk_deep_xdistance_skip_host(double A_r, double A_i, int32_t a_e, double B_r, double B_i, int32_t b_e, double *D_r, double *D_i,
                                 int32_t *e)
{
    if (!D_r || !D_i || !e) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::wide_dskip(A_r, A_i, a_e, B_r, B_i, b_e, *D_r, *D_i, *e);
    return MBK_OK;
}

// ---- count histograms and the equalisation table (mbk_histogram.h; mbk.h "Count histograms") ------------------------------

static int check_hist_mrd(mbk_ctx *ctx, uint32_t mrd)
{
    if (mrd == 0u || mrd > MBK_HISTOGRAM_MAX_MRD) return fail(ctx, MBK_ERR_INVALID, "mrd must lie in [1, MBK_HISTOGRAM_MAX_MRD]");
    return MBK_OK;
}

int mbk_counts_histogram_host(const int32_t *counts, uint64_t n, uint32_t mrd, uint64_t *hist)
{
    if (!hist || (!counts && n)) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = check_hist_mrd(nullptr, mrd);
    if (rc != MBK_OK) return rc;
    mbk::counts_histogram_host(counts, n, mrd, hist);
    return MBK_OK;
}

int mbk_equalize_lut_host(const uint64_t *hist, uint32_t mrd, double *lut)
{
    if (!hist || !lut) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    int rc = check_hist_mrd(nullptr, mrd);
    if (rc != MBK_OK) return rc;
    if (!mbk::equalize_lut_host(hist, mrd, lut))
        return fail(nullptr, MBK_ERR_INVALID, "twice the number of escaped samples must stay below 2^53");
    return MBK_OK;
}

double mbk_equalize_value_host(const double *lut, uint32_t mrd, double nu)
{
    if (!lut || mrd > MBK_HISTOGRAM_MAX_MRD) return 0.0;
    return mbk::equalize_value(lut, mrd, nu);
}

int mbk_counts_histogram(mbk_ctx *ctx, const int32_t *d_counts, uint64_t n, uint32_t mrd, uint64_t *d_hist, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    if (!d_hist || (!d_counts && n)) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    int rc = check_hist_mrd(ctx, mrd);
    if (rc != MBK_OK) return rc;
    if (((uintptr_t)d_counts & 3u) || ((uintptr_t)d_hist & 7u))
        return fail(ctx, MBK_ERR_INVALID, "d_counts must be 4-byte and d_hist 8-byte aligned");
    if (n == 0) return MBK_OK;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    mbk::launch_counts_histogram(d_counts, n, mrd, (unsigned long long *)d_hist, (uint32_t)std::max(ctx->prop.multiProcessorCount, 1),
                                 (hipStream_t)hip_stream);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

// The flags a histogram passes on to the sample launch of each kind of view, by Target::Kind
struct HistRules {
    uint32_t flags;
    const char *bad_flags;
};
static const HistRules kHistRules[4] = {
    {MBK_KERNEL_MASK | MBK_PRECISION_F32, "histogram flags carry kernel selection and MBK_PRECISION_F32 only"},
    {MBK_KERNEL_MASK, "Julia histogram flags carry kernel selection only"},
    {MBK_DEEP_BLA, "deep histograms take MBK_DEEP_BLA only (no kernel selection, no fp32)"},
    {MBK_DEEP_XBLA, "extended-range deep histograms take no flags (no MBK_DEEP_BLA, no kernel selection, no fp32)"},
};

// Everything a view histogram can refuse, before anything is allocated, enqueued or written: the sample launch's own rules.
static int hist_check(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, const void *out)
{
    if (!out) return fail(ctx, MBK_ERR_INVALID, "histogram pointer is NULL");
    if (!t.has_view) return fail(ctx, MBK_ERR_INVALID, "view is NULL");
    int rc = check_hist_mrd(ctx, mrd);
    if (rc != MBK_OK) return rc;
    if (flags & ~kHistRules[t.kind].flags) return fail(ctx, MBK_ERR_INVALID, kHistRules[t.kind].bad_flags);
    rc = target_check(ctx, t, mrd, flags | MBK_WANT_COUNTS);
    if (rc != MBK_OK) return rc;
    const uint32_t kernel = flags & MBK_KERNEL_MASK;   // (a plain view's only: no other kind takes MBK_PRECISION_F32)
    if ((flags & MBK_PRECISION_F32) && (kernel == MBK_KERNEL_SIMPLE || kernel == MBK_KERNEL_REFILL))
        return fail(ctx, MBK_ERR_INVALID, "MBK_PRECISION_F32 is implemented by the scan / asm / group kernels only");
    return MBK_OK;
}

// A checked histogram (hist_check) added into the device table d_hist, on `stream`: the window's counts band by band through
// the stream's render scratch (4 bytes per sample: the bands of render_run).  stat as for render_run: its reduction scratch
// adds up the statistics, its ev_k1 marks the last histogram kernel.
static int hist_run(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, unsigned long long *d_hist,
                    hipStream_t stream, Slot *stat)
{
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    const BandPlan plan = band_plan(t.g.ncols, t.g.nrows, 4u);
    const size_t need = plan.cap_px() * 4u;
    rc = grow(ctx, sc->d_render, sc->render_cap, need, need);
    if (rc != MBK_OK) return rc;
    int32_t *d_counts = (int32_t *)sc->d_render;   // (sc may move when a launch below adds a stream's scratch: not used past here)
    const uint32_t cus = (uint32_t)std::max(ctx->prop.multiProcessorCount, 1);
    return for_each_band(ctx, plan, d_counts, 1u, mrd, stream, stat, [&](uint32_t r, uint32_t c, uint32_t nr, uint32_t nc, bool) -> int {
        int rc = target_launch(ctx, target_samples(t, 1u, t.g.col0 + c, t.g.row0 + r, nc, nr), mrd, flags,
                               Outputs{d_counts, nullptr, nullptr, false}, stream);
        if (rc != MBK_OK) return rc;
        mbk::launch_counts_histogram(d_counts, (uint64_t)nc * nr, mrd, d_hist, cus, stream);
        MBK_HIP(ctx, hipGetLastError());
        return MBK_OK;
    });
}

static int hist_launch(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, uint64_t *d_hist, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = hist_check(ctx, t, mrd, flags, d_hist);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_hist & 7u) return fail(ctx, MBK_ERR_INVALID, "d_hist must be 8-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return hist_run(ctx, t, mrd, flags, (unsigned long long *)d_hist, (hipStream_t)hip_stream, nullptr);
}

static int hist_compute(mbk_ctx *ctx, const Target &t, uint32_t mrd, uint32_t flags, uint64_t *h_hist, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = hist_check(ctx, t, mrd, flags, h_hist);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    auto enqueue = [&]() -> int {
        int rc = grow(ctx, ctx->d_hist, ctx->hist_cap, mrd, (size_t)mrd * sizeof(uint64_t));
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipMemsetAsync(ctx->d_hist, 0, (size_t)mrd * sizeof(uint64_t), sl.stream));
        MBK_HIP(ctx, hipMemsetAsync(sl.d_red, 0, sizeof(ReduceSlot) * mbk::kReduceSlots, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
        rc = hist_run(ctx, t, mrd, flags, ctx->d_hist, sl.stream, &sl);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_hist, ctx->d_hist, (size_t)mrd * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    return sync_end(ctx, enqueue(), stats, false);
}

int mbk_view_histogram_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint64_t *d_hist, void *hip_stream)
{
    return hist_launch(ctx, view_target(view), mrd, flags, d_hist, hip_stream);
}

int mbk_view_histogram_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint64_t *h_hist, mbk_stats *stats)
{
    return hist_compute(ctx, view_target(view), mrd, flags, h_hist, stats);
}

int mbk_deep_view_histogram_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                   uint32_t flags, uint64_t *d_hist, void *hip_stream)
{
    return hist_launch(ctx, deep_target(orbit, view), mrd, flags, d_hist, hip_stream);
}

int mbk_deep_view_histogram_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                    uint32_t flags, uint64_t *h_hist, mbk_stats *stats)
{
    return hist_compute(ctx, deep_target(orbit, view), mrd, flags, h_hist, stats);
}

int mbk_deep_xview_histogram_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                    uint32_t flags, uint64_t *d_hist, void *hip_stream)
{
    return hist_launch(ctx, wide_target(orbit, view), mrd, flags, d_hist, hip_stream);
}

int mbk_deep_xview_histogram_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                     uint32_t flags, uint64_t *h_hist, mbk_stats *stats)
{
    return hist_compute(ctx, wide_target(orbit, view), mrd, flags, h_hist, stats);
}

int mbk_julia_view_histogram_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                    uint64_t *d_hist, void *hip_stream)
{
    return hist_launch(ctx, julia_target(view, c_r, c_i), mrd, flags, d_hist, hip_stream);
}

int mbk_julia_view_histogram_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                     uint64_t *h_hist, mbk_stats *stats)
{
    return hist_compute(ctx, julia_target(view, c_r, c_i), mrd, flags, h_hist, stats);
}

// ---- density views (mbk_density.h; mbk.h "Density views") ------------------------------------------------------------

// The target as the kernels take it, or what is wrong with it.  inv_* are the contract's fl(W / range_r), fl(H / range_i).
static int density_target_check(mbk_ctx *ctx, const mbk_density_target *t, mbk::DensityTarget *out)
{
    if (!t) return fail(ctx, MBK_ERR_INVALID, "density target is NULL");
    if (t->width == 0u || t->height == 0u || (uint64_t)t->width * t->height > MBK_DENSITY_MAX_CELLS)
        return fail(ctx, MBK_ERR_INVALID, "density target must hold 1 .. 2^28 cells");
    if (!std::isfinite(t->start_r) || !std::isfinite(t->start_i))
        return fail(ctx, MBK_ERR_INVALID, "density target start must be finite");
    if (!(t->range_r > 0.0) || !(t->range_i > 0.0) || !std::isfinite(t->range_r) || !std::isfinite(t->range_i))
        return fail(ctx, MBK_ERR_INVALID, "density target ranges must be finite and > 0");
    volatile double inv_r = (double)t->width / t->range_r;
    volatile double inv_i = (double)t->height / t->range_i;
    out->start_r = t->start_r;
    out->start_i = t->start_i;
    out->inv_r = inv_r;
    out->inv_i = inv_i;
    out->w = (double)t->width;
    out->h = (double)t->height;
    out->width = t->width;
    out->height = t->height;
    return MBK_OK;
}

// Everything a density launch can refuse, before anything is allocated, enqueued or written.  *minc .. *maxc: the counts that
// qualify, after the max_count == 0 substitution (with mrd < 2 no count is above 0 and the interval does not matter).
static int density_check(mbk_ctx *ctx, const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                         uint32_t max_count, uint32_t flags, mbk::DensityTarget *dt, int32_t *minc, int32_t *maxc)
{
    if (flags & ~MBK_KERNEL_MASK)
        return fail(ctx, MBK_ERR_INVALID, "density flags carry kernel selection only (no fp32, no MBK_LAZY_UNIFORM, no MBK_DEEP_BLA)");
    const uint32_t kernel = flags & MBK_KERNEL_MASK;
    if (kernel > MBK_KERNEL_SCAN) return fail(ctx, MBK_ERR_INVALID, "unknown MBK_KERNEL_* selector");
    if (kernel == MBK_KERNEL_SIMPLE || kernel == MBK_KERNEL_REFILL)
        return fail(ctx, MBK_ERR_INVALID, "density views take their counts from the scan / asm / group kernels only");
    bool dummy;
    int rc = validate_view(ctx, view, &dummy);
    if (rc != MBK_OK) return rc;
    if (mrd > 0x7fffffffu) return fail(ctx, MBK_ERR_INVALID, "mrd must fit int32 (calc_mb_value returns int32)");
    if (min_count == 0u) return fail(ctx, MBK_ERR_INVALID, "min_count must be at least 1 (a sample that never escapes deposits nothing)");
    uint32_t hi = max_count;
    if (mrd >= 2u) {
        if (max_count >= mrd) return fail(ctx, MBK_ERR_INVALID, "max_count must be below mrd");
        if (hi == 0u) hi = mrd - 1u;
    }
    if (hi != 0u && min_count > hi) return fail(ctx, MBK_ERR_INVALID, "min_count exceeds max_count");
    rc = density_target_check(ctx, target, dt);
    if (rc != MBK_OK) return rc;
    *minc = (int32_t)std::min<uint32_t>(min_count, 0x7fffffffu);
    *maxc = (int32_t)std::min<uint32_t>(hi ? hi : 0x7fffffffu, 0x7fffffffu);
    return MBK_OK;
}

// A checked density launch (density_check) added into the device table, on `stream`: the window's counts band by band through
// the stream's render scratch (4 bytes per sample, 8 with the compacted list; at most MBK_RENDER_BAND_BYTES: the bands of
// hist_run), each band replayed into the table.  d_stat: two device words for deposits / dropped points, or NULL.  stat as for
// render_run: its reduction scratch adds up the statistics of the samples, its ev_k1 marks the last replay kernel.
static int density_run(mbk_ctx *ctx, const mbk_view *v, const mbk::DensityTarget &dt, uint32_t mrd, int32_t minc, int32_t maxc,
                       uint32_t kernel, uint32_t *d_table, unsigned long long *d_stat, hipStream_t stream, Slot *stat)
{
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    const BandPlan plan = band_plan(v->ncols, v->nrows, mbk::kDensityCompact ? 8u : 4u);
    const size_t cap = plan.cap_px();
    const size_t off2 = round_up_256(cap * 4u);
    const size_t need = mbk::kDensityCompact ? off2 + cap * 4u : cap * 4u;
    rc = grow(ctx, sc->d_render, sc->render_cap, need, need);
    if (rc != MBK_OK) return rc;
    if (mbk::kDensityCompact && !sc->d_density_bands && ctx->capturing)
        return refuse_capture(ctx, "the first density call on this stream allocates its band counters: make the same call once outside the capture");
    if (mbk::kDensityCompact && !sc->d_density_bands)
        MBK_HIP(ctx, hipMalloc((void **)&sc->d_density_bands, 2u * mbk::kDensityBands * sizeof(uint32_t)));
    // (sc may move when a launch below adds a stream's scratch: not used past here)
    int32_t *d_counts = (int32_t *)sc->d_render;
    uint32_t *d_list = mbk::kDensityCompact ? (uint32_t *)((uint8_t *)sc->d_render + off2) : nullptr;
    uint32_t *d_bands = sc->d_density_bands;
    return for_each_band(ctx, plan, d_counts, 1u, mrd, stream, stat, [&](uint32_t r, uint32_t c, uint32_t nr, uint32_t nc, bool) -> int {
        mbk_view sv = *v;
        sv.col0 = v->col0 + c;
        sv.row0 = v->row0 + r;
        sv.ncols = nc;
        sv.nrows = nr;
        int rc = launch_tile(ctx, &sv, mrd, kernel | MBK_WANT_COUNTS, d_counts, nullptr, stream);
        if (rc != MBK_OK) return rc;
        if (mbk::kDensityCompact) {
            rc = clear_words(ctx, d_bands, 2u * mbk::kDensityBands, stream);
            if (rc != MBK_OK) return rc;
        }
        mbk::DensityArgs a;
        std::memset(&a, 0, sizeof(a));
        fill_window(a, &sv);
        a.min_count = minc;
        a.max_count = maxc;
        a.t = dt;
        a.counts = d_counts;
        a.table = d_table;
        a.stat = d_stat;
        a.list = d_list;
        a.bands = d_bands;
        mbk::launch_density_replay(a, stream);
        MBK_HIP(ctx, hipGetLastError());
        return MBK_OK;
    });
}

int mbk_view_density_launch(mbk_ctx *ctx, const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                            uint32_t max_count, uint32_t flags, uint32_t *d_density, void *hip_stream)
{
    if (!ctx || !d_density) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    mbk::DensityTarget dt;
    int32_t minc, maxc;
    int rc = density_check(ctx, view, target, mrd, min_count, max_count, flags, &dt, &minc, &maxc);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_density & 3u) return fail(ctx, MBK_ERR_INVALID, "d_density must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return density_run(ctx, view, dt, mrd, minc, maxc, flags & MBK_KERNEL_MASK, d_density, nullptr, (hipStream_t)hip_stream, nullptr);
}

int mbk_view_density_compute(mbk_ctx *ctx, const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                             uint32_t max_count, uint32_t flags, uint32_t *h_density, mbk_stats *stats, mbk_density_stats *dstats)
{
    if (!ctx || !h_density) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    mbk::DensityTarget dt;
    int32_t minc, maxc;
    int rc = density_check(ctx, view, target, mrd, min_count, max_count, flags, &dt, &minc, &maxc);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    const size_t cells = (size_t)dt.width * dt.height;
    unsigned long long h_stat[2] = {0ull, 0ull};
    auto enqueue = [&]() -> int {
        int rc = grow(ctx, ctx->d_density, ctx->density_cap, cells, cells * sizeof(uint32_t));
        if (rc != MBK_OK) return rc;
        if (!ctx->d_density_stat) MBK_HIP(ctx, hipMalloc((void **)&ctx->d_density_stat, 2u * sizeof(unsigned long long)));
        MBK_HIP(ctx, hipMemsetAsync(ctx->d_density, 0, cells * sizeof(uint32_t), sl.stream));
        MBK_HIP(ctx, hipMemsetAsync(ctx->d_density_stat, 0, 2u * sizeof(unsigned long long), sl.stream));
        MBK_HIP(ctx, hipMemsetAsync(sl.d_red, 0, sizeof(ReduceSlot) * mbk::kReduceSlots, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
        rc = density_run(ctx, view, dt, mrd, minc, maxc, flags & MBK_KERNEL_MASK, ctx->d_density, ctx->d_density_stat, sl.stream, &sl);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_density, ctx->d_density, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_stat, ctx->d_density_stat, sizeof(h_stat), hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    rc = sync_end(ctx, enqueue(), stats, false);
    if (rc == MBK_OK && dstats) {
        dstats->deposits = h_stat[0];
        dstats->dropped = h_stat[1];
    }
    return rc;
}

int mbk_density_max(mbk_ctx *ctx, const uint32_t *d_density, uint64_t n, uint32_t *max, uint64_t *total, void *hip_stream)
{
    if (!ctx || !max || !total || (!d_density && n)) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    if ((uintptr_t)d_density & 3u) return fail(ctx, MBK_ERR_INVALID, "d_density must be 4-byte aligned");
    *max = 0u;
    *total = 0ull;
    if (n == 0) return MBK_OK;
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (stream_capturing(s)) return refuse_capture(ctx, "mbk_density_max waits for its result and cannot be captured");
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, s, &sc);
    if (rc != MBK_OK) return rc;
    if (!sc->d_density_max) MBK_HIP(ctx, hipMalloc((void **)&sc->d_density_max, sizeof(mbk::DensityMax)));
    MBK_HIP(ctx, hipMemsetAsync(sc->d_density_max, 0, sizeof(mbk::DensityMax), s));
    const uint64_t blocks = std::min<uint64_t>((n + mbk::kDensityThreads - 1u) / mbk::kDensityThreads,
                                               (uint64_t)std::max(ctx->prop.multiProcessorCount, 1) * 8u);
    hipLaunchKernelGGL(mbk::density_max_kernel, dim3((uint32_t)blocks), dim3(mbk::kDensityThreads), 0, s, d_density, n, sc->d_density_max);
    MBK_HIP(ctx, hipGetLastError());
    mbk::DensityMax h = {};
    MBK_HIP(ctx, hipMemcpyAsync(&h, sc->d_density_max, sizeof(h), hipMemcpyDeviceToHost, s));
    MBK_HIP(ctx, hipStreamSynchronize(s));
    *max = h.max;
    *total = h.total;
    return MBK_OK;
}

// Everything a density render can refuse, before anything is allocated, enqueued or written.
static int density_render_check(mbk_ctx *ctx, const mbk_density_render_spec *spec, uint32_t width, uint32_t height, const void *table,
                                const void *out)
{
    if (!spec) return fail(ctx, MBK_ERR_INVALID, "density render spec is NULL");
    if (!spec->palette) return fail(ctx, MBK_ERR_INVALID, "palette is NULL");
    if (!table || !out) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    if (spec->mode != MBK_DENSITY_LINEAR && spec->mode != MBK_DENSITY_SQRT) return fail(ctx, MBK_ERR_INVALID, "unknown MBK_DENSITY_* mode");
    const uint32_t k = spec->factor;
    if (k != 1u && k != 2u && k != 4u && k != 8u) return fail(ctx, MBK_ERR_INVALID, "factor must be 1, 2, 4 or 8");
    if (spec->palette_len < 2u || spec->palette_len > 65536u) return fail(ctx, MBK_ERR_INVALID, "a density render takes a palette of 2 .. 65536 entries");
    if (!(spec->scale > 0.0) || !(spec->scale <= 0x1p80)) return fail(ctx, MBK_ERR_INVALID, "scale must lie in (0, 2^80]");
    if (!(std::fabs(spec->offset) <= 0x1p20)) return fail(ctx, MBK_ERR_INVALID, "offset must lie in [-2^20, 2^20]");
    if (width == 0u || height == 0u || (uint64_t)width * height > MBK_DENSITY_MAX_CELLS)
        return fail(ctx, MBK_ERR_INVALID, "a density table holds 1 .. 2^28 cells");
    if (width % k || height % k) return fail(ctx, MBK_ERR_INVALID, "width and height must be multiples of factor");
    return MBK_OK;
}

static mbk::RenderPalette density_palette(const mbk_density_render_spec *spec, const uint32_t *entries)
{
    mbk::RenderPalette p;
    std::memset(&p, 0, sizeof(p));
    p.entries = entries;
    p.n = spec->palette_len;
    p.n_rcp = 1.0 / (double)spec->palette_len;
    p.scale = spec->scale;
    p.offset = spec->offset;
    return p;
}

// A checked density render of the device table onto the device image d_out ((height / k) x (width / k) words), on `stream`.
static int density_render_run(mbk_ctx *ctx, const uint32_t *d_table, uint32_t width, uint32_t height, const mbk_density_render_spec *spec,
                              uint32_t *d_out, hipStream_t stream)
{
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    rc = stream_palette(ctx, sc, stream, spec->palette, spec->palette_len);
    if (rc != MBK_OK) return rc;
    mbk::DensityResolveArgs a;
    std::memset(&a, 0, sizeof(a));
    a.table = d_table;
    a.out = d_out;
    a.width = width;
    a.out_w = width / spec->factor;
    a.out_h = height / spec->factor;
    a.root = spec->mode == MBK_DENSITY_SQRT ? 1u : 0u;
    a.pal = density_palette(spec, sc->d_palette);
    const uint64_t px = (uint64_t)a.out_w * a.out_h;
    const uint64_t blocks = std::min<uint64_t>((px + mbk::kDensityThreads - 1u) / mbk::kDensityThreads,
                                               (uint64_t)std::max(ctx->prop.multiProcessorCount, 1) * 8u);
    mbk::launch_density_resolve(spec->factor, dim3((uint32_t)blocks), stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

int mbk_density_render_launch(mbk_ctx *ctx, const uint32_t *d_density, uint32_t width, uint32_t height,
                              const mbk_density_render_spec *spec, uint8_t *d_rgba, void *hip_stream)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = density_render_check(ctx, spec, width, height, d_density, d_rgba);
    if (rc != MBK_OK) return rc;
    if (((uintptr_t)d_density & 3u) || ((uintptr_t)d_rgba & 3u)) return fail(ctx, MBK_ERR_INVALID, "d_density and d_rgba must be 4-byte aligned");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    CaptureScope capture(ctx, (hipStream_t)hip_stream);
    return density_render_run(ctx, d_density, width, height, spec, (uint32_t *)d_rgba, (hipStream_t)hip_stream);
}

int mbk_density_render_compute(mbk_ctx *ctx, const uint32_t *h_density, uint32_t width, uint32_t height,
                               const mbk_density_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats)
{
    if (!ctx) return fail(ctx, MBK_ERR_INVALID, "ctx is NULL");
    int rc = density_render_check(ctx, spec, width, height, h_density, h_rgba);
    if (rc != MBK_OK) return rc;
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    const size_t cells = (size_t)width * height, px = cells / ((size_t)spec->factor * spec->factor);
    auto enqueue = [&]() -> int {
        int rc = grow(ctx, ctx->d_density, ctx->density_cap, cells, cells * sizeof(uint32_t));
        if (rc == MBK_OK) rc = grow(ctx, ctx->d_rgba, ctx->rgba_cap_px, px, px * sizeof(uint32_t));
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipMemcpyAsync(ctx->d_density, h_density, cells * sizeof(uint32_t), hipMemcpyHostToDevice, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_k0, sl.stream));
        rc = density_render_run(ctx, ctx->d_density, width, height, spec, ctx->d_rgba, sl.stream);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_k1, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_rgba, ctx->d_rgba, px * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    return sync_end(ctx, enqueue(), stats, false, false);
}

int mbk_density_cell_host(const mbk_density_target *target, double z_r, double z_i, uint32_t *cell_x, uint32_t *cell_y, int *inside)
{
    if (!cell_x || !cell_y || !inside) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::DensityTarget dt;
    int rc = density_target_check(nullptr, target, &dt);
    if (rc != MBK_OK) return rc;
    uint32_t cx = 0u, cy = 0u;
    *inside = mbk::density_cell(dt, z_r, z_i, &cx, &cy) ? 1 : 0;
    *cell_x = cx;
    *cell_y = cy;
    return MBK_OK;
}

int mbk_density_accumulate_host(const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                                uint32_t max_count, uint32_t *density, mbk_density_stats *dstats)
{
    if (!density) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbk::DensityTarget dt;
    int32_t minc, maxc;
    int rc = density_check(nullptr, view, target, mrd, min_count, max_count, 0u, &dt, &minc, &maxc);
    if (rc != MBK_OK) return rc;
    const Axis re = make_axis(view->start_r, view->range_r, view->width), im = make_axis(view->start_i, view->range_i, view->height);
    std::vector<double> cr(view->ncols), ci(view->nrows);
    for (uint32_t c = 0; c < view->ncols; ++c) cr[c] = axis_value_host(re, view->col0 + c);
    for (uint32_t r = 0; r < view->nrows; ++r) ci[r] = axis_value_host(im, view->row0 + r);
    std::vector<int32_t> counts((size_t)view->ncols * view->nrows);
    for (uint32_t r = 0; r < view->nrows; ++r)
        for (uint32_t c = 0; c < view->ncols; ++c) {
            double m;
            counts[(size_t)r * view->ncols + c] = mbk::julia_count<false>(cr[c], ci[r], cr[c], ci[r], (int32_t)mrd, &m);
        }
    uint64_t deposits = 0, dropped = 0;
    mbk::density_accumulate_host(cr.data(), ci.data(), view->ncols, view->nrows, counts.data(), minc, maxc, dt, density, &deposits, &dropped);
    if (dstats) {
        dstats->deposits = deposits;
        dstats->dropped = dropped;
    }
    return MBK_OK;
}

int mbk_density_build_info(void) { return MBK_DENSITY_COMPACT; }

int mbk_density_resolve_host(const mbk_density_render_spec *spec, uint32_t width, uint32_t height, const uint32_t *density, uint8_t *rgba)
{
    int rc = density_render_check(nullptr, spec, width, height, density, rgba);
    if (rc != MBK_OK) return rc;
    std::vector<uint32_t> words(spec->palette_len);
    for (uint32_t k = 0; k < spec->palette_len; ++k) words[k] = pack_rgba(spec->palette + 4u * (size_t)k);
    mbk::density_resolve_host(density_palette(spec, words.data()), spec->mode == MBK_DENSITY_SQRT, spec->factor, width, height, density, rgba);
    return MBK_OK;
}

// ---- the native worker loop (mbk_feeder.h) ----------------------------------------------------------------

// ---- stored chunks (mbk_chunks.h; mbk.h "Stored chunks") ------------------------------------------------------------

static const char *stream_reason_text(uint32_t reason)
{
    switch (reason) {
        case MBK_STREAM_OK: return "MBK_STREAM_OK";
        case MBK_STREAM_BAD_CODEC: return "MBK_STREAM_BAD_CODEC: the code byte is neither Raw nor RLE";
        case MBK_STREAM_BAD_SIZE: return "MBK_STREAM_BAD_SIZE: empty stream, Raw shorter than 1 + n, RLE payload not a multiple of 5 or longer than n";
        case MBK_STREAM_ZERO_RUN: return "MBK_STREAM_ZERO_RUN: a run of length 0";
        case MBK_STREAM_TOO_LONG: return "MBK_STREAM_TOO_LONG: the run lengths sum to more than n";
        case MBK_STREAM_TOO_SHORT: return "MBK_STREAM_TOO_SHORT: the run lengths sum to less than n";
    }
    return "unknown MBK_STREAM_* reason";
}

static int fail_stream(mbk_ctx *ctx, uint32_t reason) { return fail(ctx, MBK_ERR_INVALID, std::string("invalid chunk stream: ") + stream_reason_text(reason)); }

static uint32_t record_length(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// What can be said about a stream without walking its payload: the reason code (MBK_STREAM_OK = nothing against it so far),
// the code byte and the number of RLE records.  A stream of one record is judged completely.
static uint32_t stream_precheck(const uint8_t *stream, uint64_t size, uint64_t n, uint32_t *codec, uint64_t *runs)
{
    *codec = 0;
    *runs = 0;
    if (size == 0 || n == 0 || n > MBK_CHUNK_BYTES) return MBK_STREAM_BAD_SIZE;
    *codec = stream[0];
    if (stream[0] == MBK_CODEC_RAW) return size >= 1 + n ? MBK_STREAM_OK : MBK_STREAM_BAD_SIZE;
    if (stream[0] != MBK_CODEC_RLE) return MBK_STREAM_BAD_CODEC;
    if ((size - 1) % 5 != 0 || size > 1 + n) return MBK_STREAM_BAD_SIZE;
    *runs = (size - 1) / 5;
    if (*runs == 0) return MBK_STREAM_TOO_SHORT;
    if (*runs == 1) return mbk::chunk_status_of(record_length(stream + 1) == 0, record_length(stream + 1), n);
    return MBK_STREAM_OK;
}

static int chunk_scale_log2(uint32_t k)
{
    for (int lk = 0; lk <= 6; ++lk)
        if (k == (1u << lk)) return lk;
    return -1;
}

int mbk_chunk_stream_check(const uint8_t *stream, uint64_t size, uint64_t n, uint32_t *codec, uint64_t *runs, uint32_t *reason)
{
    if (!stream) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    uint32_t c;
    uint64_t r;
    uint32_t why = stream_precheck(stream, size, n, &c, &r);
    if (why == MBK_STREAM_OK && r > 1) why = mbk::chunk_check_records_host(stream + 1, r, n);
    if (codec) *codec = c;
    if (runs) *runs = r;
    if (reason) *reason = why;
    return why == MBK_STREAM_OK ? MBK_OK : fail_stream(nullptr, why);
}

int mbk_chunk_decode_host(const uint8_t *stream, uint64_t size, uint64_t n, uint8_t *bytes)
{
    if (!bytes) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    uint32_t codec;
    uint64_t runs;
    const int rc = mbk_chunk_stream_check(stream, size, n, &codec, &runs, nullptr);
    if (rc != MBK_OK) return rc;
    if (codec == MBK_CODEC_RAW)
        std::memcpy(bytes, stream + 1, n);
    else
        mbk::chunk_expand_host(stream + 1, runs, bytes);
    return MBK_OK;
}

static int validate_chunk_spec(mbk_ctx *ctx, const mbk_chunk_spec *spec, const void *out, uint64_t pitch_px, int *lk)
{
    if (!spec || !spec->palette || !out) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    *lk = chunk_scale_log2(spec->scale);
    if (*lk < 0) return fail(ctx, MBK_ERR_INVALID, "scale must be 1, 2, 4, 8, 16, 32 or 64");
    if (pitch_px < (MBK_CHUNK_DEFINITION >> *lk) || pitch_px > (1ull << 40))
        return fail(ctx, MBK_ERR_INVALID, "pitch_px must be at least 4096 / scale");
    return MBK_OK;
}

int mbk_chunk_resolve_host(const mbk_chunk_spec *spec, const uint8_t *bytes, uint8_t *rgba, uint64_t pitch_px)
{
    int lk;
    const int rc = validate_chunk_spec(nullptr, spec, rgba, pitch_px, &lk);
    if (rc != MBK_OK) return rc;
    if (!bytes) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    uint32_t words[256];
    for (uint32_t k = 0; k < 256u; ++k) words[k] = pack_rgba(spec->palette + 4u * k);
    mbk::chunk_resolve_host(words, (uint32_t)lk, bytes, rgba, pitch_px);
    return MBK_OK;
}

// The parts of a stream's chunk scratch for n output bytes (all on 256-byte lines).
struct ChunkScratch {
    uint32_t *words;                  // the payload: at most n bytes, read in groups of 20
    uint32_t *starts;                 // n / 5 records, in whole groups of four
    uint8_t *values;
    unsigned long long *block_sum;
    uint32_t *block_zero, *state;
    size_t total;
};
static ChunkScratch chunk_scratch_layout(uint8_t *base, size_t n)
{
    const size_t recs = (n / 5u + 4u) & ~(size_t)3u, blocks = recs / mbk::kChunkScanRecords + 1u;
    size_t off = 0;
    ChunkScratch c;
    c.words = (uint32_t *)(base + off);
    off = round_up_256(off + n + 32u);
    c.starts = (uint32_t *)(base + off);
    off = round_up_256(off + recs * 4u);
    c.values = base + off;
    off = round_up_256(off + recs);
    c.block_sum = (unsigned long long *)(base + off);
    off = round_up_256(off + blocks * 8u);
    c.block_zero = (uint32_t *)(base + off);
    off = round_up_256(off + blocks * 4u);
    c.state = (uint32_t *)(base + off);
    c.total = off + 256u;
    return c;
}

// A prechecked stream (stream_precheck: MBK_STREAM_OK) decoded into d_bytes[n] on `stream`; the reason code goes to d_status
// (may be NULL) and, with h_status (pinned), to the host.  ev_k0 (may be NULL) is recorded behind the upload of the stream:
// where the kernel time of the synchronous forms starts.
static int chunk_decode_run(mbk_ctx *ctx, StreamScratch *sc, const uint8_t *h_stream, uint64_t size, uint64_t n, uint32_t codec,
                            uint64_t runs, uint8_t *d_bytes, uint32_t *d_status, uint32_t *h_status, hipEvent_t ev_k0,
                            hipStream_t stream)
{
    if (codec == MBK_CODEC_RAW || runs == 1) {
        if (codec == MBK_CODEC_RAW)
            MBK_HIP(ctx, hipMemcpyAsync(d_bytes, h_stream + 1, n, hipMemcpyHostToDevice, stream));
        if (ev_k0) MBK_HIP(ctx, hipEventRecord(ev_k0, stream));
        if (codec != MBK_CODEC_RAW)
            MBK_HIP(ctx, hipMemsetAsync(d_bytes, h_stream[5], n, stream));
        if (d_status) MBK_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(uint32_t), stream));
        if (h_status) *h_status = MBK_STREAM_OK;
        return MBK_OK;
    }
    if (n > sc->chunk_cap_n) {
        if (sc->d_chunk) (void)hipFree(sc->d_chunk);   // (hipFree waits for the launches that may still read it)
        sc->d_chunk = nullptr;
        sc->chunk_cap_n = 0;
        MBK_HIP(ctx, hipMalloc((void **)&sc->d_chunk, chunk_scratch_layout(nullptr, n).total));
        sc->chunk_cap_n = n;
    }
    const ChunkScratch c = chunk_scratch_layout(sc->d_chunk, sc->chunk_cap_n);
    MBK_HIP(ctx, hipMemcpyAsync(c.words, h_stream + 1, size - 1, hipMemcpyHostToDevice, stream));
    if (ev_k0) MBK_HIP(ctx, hipEventRecord(ev_k0, stream));
    const uint32_t r = (uint32_t)runs, nblocks = (r + mbk::kChunkScanRecords - 1u) / mbk::kChunkScanRecords;
    hipLaunchKernelGGL(mbk::chunk_block_sums_kernel, dim3(nblocks), dim3(mbk::kChunkScanThreads), 0, stream, c.words, r, c.block_sum,
                       c.block_zero);
    hipLaunchKernelGGL(mbk::chunk_scan_sums_kernel, dim3(1), dim3(1024), 0, stream, c.block_sum, c.block_zero, nblocks,
                       (unsigned long long)n, c.state, d_status);
    hipLaunchKernelGGL(mbk::chunk_starts_kernel, dim3(nblocks), dim3(mbk::kChunkScanThreads), 0, stream, c.words, r, c.block_sum,
                       (unsigned long long)n, c.starts, (uint32_t *)c.values);
    hipLaunchKernelGGL(mbk::chunk_expand_kernel, dim3((uint32_t)((n + mbk::kChunkPiece - 1u) / mbk::kChunkPiece)), dim3(256), 0, stream,
                       c.starts, c.values, r, (uint32_t)n, d_bytes);
    MBK_HIP(ctx, hipGetLastError());
    if (h_status) MBK_HIP(ctx, hipMemcpyAsync(h_status, c.state, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return MBK_OK;
}

// A prechecked stream of a whole chunk rendered to d_out (rows of `pitch` pixels) on `stream`.
static int chunk_render_run(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, uint32_t codec, uint64_t runs,
                            const mbk_chunk_spec *spec, int lk, uint32_t *d_out, uint64_t pitch, uint32_t *d_status,
                            bool want_h_status, uint32_t **h_status, hipEvent_t ev_k0, hipStream_t stream)
{
    StreamScratch *sc = nullptr;
    int rc = get_scratch(ctx, stream, &sc);
    if (rc != MBK_OK) return rc;
    if (want_h_status && !sc->h_chunk_status) MBK_HIP(ctx, hipHostMalloc((void **)&sc->h_chunk_status, sizeof(uint32_t), hipHostMallocDefault));
    if (h_status) *h_status = sc->h_chunk_status;
    const uint32_t w = MBK_CHUNK_DEFINITION >> lk;
    if (codec == MBK_CODEC_RLE && runs == 1) {   // a chunk of one value: no decode, no palette upload
        if (ev_k0) MBK_HIP(ctx, hipEventRecord(ev_k0, stream));
        hipLaunchKernelGGL(mbk::chunk_fill_kernel, dim3((w * (w / 4u) + 255u) / 256u), dim3(256), 0, stream, d_out, pitch, w,
                           pack_rgba(spec->palette + 4u * (size_t)h_stream[5]));
        MBK_HIP(ctx, hipGetLastError());
        if (d_status) MBK_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(uint32_t), stream));
        if (want_h_status) *sc->h_chunk_status = MBK_STREAM_OK;
        return MBK_OK;
    }
    rc = stream_palette(ctx, sc, stream, spec->palette, 256u);
    if (rc != MBK_OK) return rc;
    if (!sc->d_chunk_bytes) MBK_HIP(ctx, hipMalloc((void **)&sc->d_chunk_bytes, MBK_CHUNK_BYTES));
    rc = chunk_decode_run(ctx, sc, h_stream, size, MBK_CHUNK_BYTES, codec, runs, sc->d_chunk_bytes, d_status,
                          want_h_status ? sc->h_chunk_status : nullptr, ev_k0, stream);
    if (rc != MBK_OK) return rc;
    mbk::ChunkRenderArgs a;
    a.bytes = sc->d_chunk_bytes;
    a.palette = sc->d_palette;
    a.out = d_out;
    a.pitch = pitch;
    mbk::launch_chunk_resolve((uint32_t)lk, stream, a);
    MBK_HIP(ctx, hipGetLastError());
    return MBK_OK;
}

int mbk_chunk_decode_launch(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, uint64_t n, uint8_t *d_bytes,
                            uint32_t *d_status, void *hip_stream)
{
    if (!ctx || !h_stream || !d_bytes) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    uint32_t codec;
    uint64_t runs;
    const uint32_t why = stream_precheck(h_stream, size, n, &codec, &runs);
    if (why != MBK_STREAM_OK) return fail_stream(ctx, why);
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    if (stream_capturing((hipStream_t)hip_stream))
        return refuse_capture(ctx, "mbk_chunk_decode_launch reads its input from host memory at enqueue time and cannot be captured");
    StreamScratch *sc = nullptr;
    const int rc = get_scratch(ctx, (hipStream_t)hip_stream, &sc);
    if (rc != MBK_OK) return rc;
    return chunk_decode_run(ctx, sc, h_stream, size, n, codec, runs, d_bytes, d_status, nullptr, nullptr, (hipStream_t)hip_stream);
}

int mbk_chunk_render_launch(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, const mbk_chunk_spec *spec, uint8_t *d_rgba,
                            uint64_t pitch_px, uint32_t *d_status, void *hip_stream)
{
    if (!ctx || !h_stream) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    int lk;
    const int rc = validate_chunk_spec(ctx, spec, d_rgba, pitch_px, &lk);
    if (rc != MBK_OK) return rc;
    if ((uintptr_t)d_rgba & 3u) return fail(ctx, MBK_ERR_INVALID, "d_rgba must be 4-byte aligned");
    uint32_t codec;
    uint64_t runs;
    const uint32_t why = stream_precheck(h_stream, size, MBK_CHUNK_BYTES, &codec, &runs);
    if (why != MBK_STREAM_OK) return fail_stream(ctx, why);
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    if (stream_capturing((hipStream_t)hip_stream))
        return refuse_capture(ctx, "mbk_chunk_render_launch reads its input from host memory at enqueue time and cannot be captured");
    return chunk_render_run(ctx, h_stream, size, codec, runs, spec, lk, (uint32_t *)d_rgba, pitch_px, d_status, false, nullptr,
                            nullptr, (hipStream_t)hip_stream);
}

int mbk_chunk_decode_compute(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, uint64_t n, uint8_t *h_bytes, mbk_stats *stats)
{
    if (!ctx || !h_stream || !h_bytes) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    uint32_t codec;
    uint64_t runs;
    const uint32_t why = stream_precheck(h_stream, size, n, &codec, &runs);
    if (why != MBK_STREAM_OK) return fail_stream(ctx, why);
    int rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    StreamScratch *sc = nullptr;
    auto decode = [&]() -> int {
        int rc = get_scratch(ctx, sl.stream, &sc);
        if (rc != MBK_OK) return rc;
        if (!sc->h_chunk_status) MBK_HIP(ctx, hipHostMalloc((void **)&sc->h_chunk_status, sizeof(uint32_t), hipHostMallocDefault));
        // the decoded bytes live in the stream's scratch, not in the slot's tile buffer: mbk_serialize_last is not affected
        if (!sc->d_chunk_bytes) MBK_HIP(ctx, hipMalloc((void **)&sc->d_chunk_bytes, MBK_CHUNK_BYTES));
        rc = chunk_decode_run(ctx, sc, h_stream, size, n, codec, runs, sc->d_chunk_bytes, nullptr, sc->h_chunk_status, sl.ev_k0, sl.stream);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_k1, sl.stream));
        return launch_reduce(ctx, sl, nullptr, sc->d_chunk_bytes, n, 0u, sl.stream);
    };
    // the verdict on the stream first: a bad one leaves h_bytes untouched
    rc = sync_end(ctx, decode(), nullptr, false);
    if (rc != MBK_OK) return rc;
    if (*sc->h_chunk_status != MBK_STREAM_OK) return fail_stream(ctx, *sc->h_chunk_status);
    auto copy = [&]() -> int {
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        MBK_HIP(ctx, hipMemcpyAsync(h_bytes, sc->d_chunk_bytes, n, hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    return sync_end(ctx, copy(), stats, true);
}

int mbk_chunk_render_compute(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, const mbk_chunk_spec *spec, uint8_t *h_rgba,
                             uint64_t pitch_px, mbk_stats *stats)
{
    if (!ctx || !h_stream) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    int lk;
    int rc = validate_chunk_spec(ctx, spec, h_rgba, pitch_px, &lk);
    if (rc != MBK_OK) return rc;
    uint32_t codec;
    uint64_t runs;
    const uint32_t why = stream_precheck(h_stream, size, MBK_CHUNK_BYTES, &codec, &runs);
    if (why != MBK_STREAM_OK) return fail_stream(ctx, why);
    rc = sync_begin(ctx);
    if (rc != MBK_OK) return rc;
    Slot &sl = ctx->s[0];
    const uint32_t w = MBK_CHUNK_DEFINITION >> lk;
    const size_t px = (size_t)w * w;
    uint32_t *h_status = nullptr;
    auto render = [&]() -> int {
        int rc = grow(ctx, ctx->d_rgba, ctx->rgba_cap_px, px, px * sizeof(uint32_t));
        if (rc != MBK_OK) return rc;
        rc = chunk_render_run(ctx, h_stream, size, codec, runs, spec, lk, ctx->d_rgba, w, nullptr, true, &h_status, sl.ev_k0, sl.stream);
        if (rc != MBK_OK) return rc;
        MBK_HIP(ctx, hipEventRecord(sl.ev_k1, sl.stream));
        return MBK_OK;
    };
    // the verdict on the stream first: a bad one leaves h_rgba untouched
    rc = sync_end(ctx, render(), nullptr, false);
    if (rc != MBK_OK) return rc;
    if (*h_status != MBK_STREAM_OK) return fail_stream(ctx, *h_status);
    auto copy = [&]() -> int {
        MBK_HIP(ctx, hipEventRecord(sl.ev_c0, sl.stream));
        if (pitch_px == w)
            MBK_HIP(ctx, hipMemcpyAsync(h_rgba, ctx->d_rgba, px * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
        else
            MBK_HIP(ctx, hipMemcpy2DAsync(h_rgba, pitch_px * sizeof(uint32_t), ctx->d_rgba, (size_t)w * sizeof(uint32_t),
                                          (size_t)w * sizeof(uint32_t), w, hipMemcpyDeviceToHost, sl.stream));
        MBK_HIP(ctx, hipEventRecord(sl.ev_c1, sl.stream));
        return MBK_OK;
    };
    return sync_end(ctx, copy(), stats, false, false);   // (no statistics of the bytes: nothing was reduced)
}

static int ctx_submit(void *user, int slot, uint32_t level, uint32_t mrd, uint32_t ir, uint32_t ii, uint8_t *h_bytes)
{
    return mbk_datachunk_submit_ex((mbk_ctx *)user, slot, level, mrd, ir, ii, h_bytes, nullptr, MBK_LAZY_UNIFORM);
}
static int ctx_wait(void *user, int slot, mbk_stats *stats) { return mbk_wait((mbk_ctx *)user, slot, stats); }
static void *ctx_alloc(void *user, uint64_t bytes)
{
    void *p = nullptr;
    return mbk_host_alloc((mbk_ctx *)user, bytes, &p) == MBK_OK ? p : nullptr;
}
static void ctx_release(void *user, void *ptr) { (void)mbk_host_free((mbk_ctx *)user, ptr); }

int mbk_net_set_option(int option, uint32_t value)
{
    mbkf::NetConfig &c = mbkf::net();
    switch (option) {
        case MBK_NET_MAX_CONNECTIONS:
            if (value < 1u || value > 64u) return fail(nullptr, MBK_ERR_INVALID, "max connections must be in 1..64");
            c.max_connections.store(value);
            {
                std::lock_guard<std::mutex> g(c.m);
                c.peak = c.open;
            }
            c.cv.notify_all();
            return MBK_OK;
        case MBK_NET_CONNECT_TIMEOUT_MS: c.connect_timeout_ms.store(value); return MBK_OK;
        case MBK_NET_IO_TIMEOUT_MS: c.io_timeout_ms.store(value); return MBK_OK;
        case MBK_NET_RETRIES:
            if (value > 100u) return fail(nullptr, MBK_ERR_INVALID, "retries must be in 0..100");
            c.retries.store(value);
            return MBK_OK;
        case MBK_NET_BACKOFF_MS:
            if (value < 1u || value > 10000u) return fail(nullptr, MBK_ERR_INVALID, "backoff must be in 1..10000 ms");
            c.backoff_ms.store(value);
            return MBK_OK;
        case MBK_NET_STOP: c.stop.store(value ? 1u : 0u); return MBK_OK;
        case MBK_NET_FEEDER_SLOTS:
            if (value < 1u || value > 8u) return fail(nullptr, MBK_ERR_INVALID, "feeder slots must be in 1..8");
            c.feeder_slots.store(value);
            return MBK_OK;
        default: return fail(nullptr, MBK_ERR_INVALID, "unknown MBK_NET_* selector");
    }
}

int mbk_net_get_option(int option, uint32_t *value)
{
    if (!value) return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    mbkf::NetConfig &c = mbkf::net();
    switch (option) {
        case MBK_NET_MAX_CONNECTIONS: *value = c.max_connections.load(); return MBK_OK;
        case MBK_NET_CONNECT_TIMEOUT_MS: *value = c.connect_timeout_ms.load(); return MBK_OK;
        case MBK_NET_IO_TIMEOUT_MS: *value = c.io_timeout_ms.load(); return MBK_OK;
        case MBK_NET_RETRIES: *value = c.retries.load(); return MBK_OK;
        case MBK_NET_BACKOFF_MS: *value = c.backoff_ms.load(); return MBK_OK;
        case MBK_NET_STOP: *value = c.stop.load(); return MBK_OK;
        case MBK_NET_FEEDER_SLOTS: *value = c.feeder_slots.load(); return MBK_OK;
        case MBK_NET_PEAK_CONNECTIONS: {
            std::lock_guard<std::mutex> g(c.m);
            *value = c.peak;
            return MBK_OK;
        }
        default: return fail(nullptr, MBK_ERR_INVALID, "unknown MBK_NET_* selector");
    }
}

int mbk_feeder_run(const mbk_feeder_ops *ops, const char *addr, uint16_t port, uint64_t max_tiles, uint32_t senders,
                   mbk_worker_report *report)
{
    if (!ops || !ops->submit || !ops->wait || !ops->alloc || !ops->release || !addr)
        return fail(nullptr, MBK_ERR_INVALID, "NULL argument");
    std::string err;
    const int rc = mbkf::run(ops, addr, port, max_tiles, senders, report, &err, mbkf::net().feeder_slots.load());
    if (rc != MBK_OK) return fail(nullptr, rc, err);
    return MBK_OK;
}

int mbk_worker_run(mbk_ctx *ctx, const char *addr, uint16_t port, uint64_t max_tiles, uint32_t senders,
                   mbk_worker_report *report)
{
    if (!ctx || !addr) return fail(ctx, MBK_ERR_INVALID, "NULL argument");
    for (Slot &sl : ctx->s)
        if (sl.busy) return fail(ctx, MBK_ERR_INVALID, "a slot still has a tile in flight: call mbk_wait first");
    MBK_HIP(ctx, hipSetDevice(ctx->device));
    mbk_feeder_ops ops;
    ops.user = ctx;
    ops.submit = ctx_submit;
    ops.wait = ctx_wait;
    ops.alloc = ctx_alloc;
    ops.release = ctx_release;
    ops.on_tile = nullptr;
    std::string err;
    const int rc = mbkf::run(&ops, addr, port, max_tiles, senders, report, &err, (uint32_t)MBK_WORKER_DEPTH);
    if (rc != MBK_OK) {
        // a backend failure left its own message on the ctx; keep it, prefixed
        const std::string inner = ctx->err;
        return fail(ctx, rc, inner.empty() || rc == MBK_ERR_NET ? err : err + ": " + inner);
    }
    return MBK_OK;
}

}  // extern "C"
