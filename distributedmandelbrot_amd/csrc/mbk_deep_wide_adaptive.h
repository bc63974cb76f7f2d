// mbk_deep_wide_adaptive.h -- adaptive supersampling of extended-range deep-view smooth renders (include/mbk.h, "Adaptive
// supersampling of extended-range deep views"): the refine kernel.  The base pass is the wide sample launch and the classify
// kernel is mbk_adaptive.h's, which works on samples and does not care what kind of view made them; what a wide view needs of
// its own is the sampler that computes a fine sample of a listed pixel in the wide number system.
//
// The list is walked by adaptive_walk (mbk_adaptive.h, which states the sampler contract).  Every lane of the wave calls the
// sampler; a lane with a sample takes dcm of sample (k_r, k_i) of the (W s) x (H s) view from deep_offset, as deep_pixel does,
// and runs deep_wide_escape or, with a table, deep_wide_bla_escape -- the loops of deep_wide_kernel and deep_wide_bla_kernel
// themselves, so count and |z|^2 are the bits mbk_deep_xview_launch stores for that sample.  The loop runs inside `if (valid)`:
// an ordinary divergent loop in which a lane without a sample executes no step and from which no wave-uniform value is taken.
// Nothing in this sampler is wave-uniform but the arguments.
#pragma once

#include "mbk_adaptive.h"
#include "mbk_deep_wide_bla.h"

namespace mbk {

struct DeepWideAdaptiveRefineArgs {
    AdaptiveWalkArgs w;
    DeepWideBlaArgs b;       // b.v: the wide orbit, exp2 and the window (col0 .. nrows) of the (W s) x (H s) view that holds the
                             // band's fine samples (fill_deep_window); no outputs.  The table (ke, ab, levels, off) with kXbla only.
};

// kXbla false: deep_wide_kernel's loop (any M); true: deep_wide_bla_kernel's (M >= 2).  The plain loop goes through the shared
// function although that costs this kernel 0.9 % at s = 8 against the three copies it replaced (one instruction more in the
// loop's 80): a copy of the loop kept here for this kernel alone, with reference out-parameters, has the old 80 and measured
// 4.3 % SLOWER at s = 8 (profiles/refine_walk/README.md, section 4).
template <int S, bool kXbla>
__global__ __launch_bounds__(256) void deep_wide_adaptive_refine_kernel(const DeepWideAdaptiveRefineArgs a)
{
    adaptive_walk<S>(a.w, a.b.v.mrd, [&a](bool valid, uint32_t row, uint32_t col, uint32_t sx, uint32_t sy) {
        EscapeSample f = {0, 0.0};
        if (valid) {
            double dcr, dci;
            deep_offset(a.b.v, col * (uint32_t)S + sx, row * (uint32_t)S + sy, dcr, dci);
            if constexpr (kXbla) f = deep_wide_bla_escape(a.b, dcr, dci);
            else f = deep_wide_escape(a.b.v, dcr, dci);
        }
        return f;
    });
}

template <bool kXbla>
struct DeepWideAdaptiveRefine {
    using Args = DeepWideAdaptiveRefineArgs;
    template <int S>
    static constexpr auto kernel = deep_wide_adaptive_refine_kernel<S, kXbla>;
};

}   // namespace mbk
