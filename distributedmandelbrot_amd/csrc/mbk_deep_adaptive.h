// mbk_deep_adaptive.h -- adaptive supersampling of deep-view smooth renders (include/mbk.h, "Adaptive supersampling of deep
// views"): the refine kernel.  The base pass is the deep sample launch and the classify kernel is mbk_adaptive.h's, which works
// on samples and does not care what kind of view made them; what a deep view needs of its own is the sampler that computes a
// fine sample of a listed pixel by perturbation.
//
// The list is walked by adaptive_walk (mbk_adaptive.h, which states the sampler contract).  Every lane of the wave calls the
// sampler; a lane with a sample takes dc of sample (k_r, k_i) of the (W s) x (H s) view from deep_offset, as deep_pixel does,
// and runs deep_escape or, with a table, deep_bla_escape -- the loops of deep_view_kernel and deep_bla_kernel themselves, so
// count and |z|^2 are the bits mbk_deep_view_launch stores for that sample.  The loop runs inside `if (valid)`: an ordinary
// divergent loop in which a lane without a sample executes no step and from which no wave-uniform value is taken.  Nothing in
// this sampler is wave-uniform but the arguments.
#pragma once

#include "mbk_adaptive.h"
#include "mbk_deep_bla.h"

namespace mbk {

struct DeepAdaptiveRefineArgs {
    AdaptiveWalkArgs w;
    DeepBlaArgs b;           // b.v: the orbit and the window (col0 .. nrows) of the (W s) x (H s) view that holds the band's
                             // fine samples (fill_deep_window); no outputs.  The table (rc, ab, levels, off) with kBla only.
};

// kBla false: deep_view_kernel's loop (any M); true: deep_bla_kernel's (M >= 2)
template <int S, bool kBla>
__global__ __launch_bounds__(256) void deep_adaptive_refine_kernel(const DeepAdaptiveRefineArgs q)
{
    adaptive_walk<S>(q.w, q.b.v.mrd, [&q](bool valid, uint32_t row, uint32_t col, uint32_t sx, uint32_t sy) {
        EscapeSample f = {0, 0.0};
        if (valid) {
            double dcr, dci;
            deep_offset(q.b.v, col * (uint32_t)S + sx, row * (uint32_t)S + sy, dcr, dci);
            if constexpr (kBla) f = deep_bla_escape(q.b, dcr, dci);
            else f = deep_escape(q.b.v, dcr, dci);
        }
        return f;
    });
}

template <bool kBla>
struct DeepAdaptiveRefine {
    using Args = DeepAdaptiveRefineArgs;
    template <int S>
    static constexpr auto kernel = deep_adaptive_refine_kernel<S, kBla>;
};

}   // namespace mbk
