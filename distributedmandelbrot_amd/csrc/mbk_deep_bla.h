// mbk_deep_bla.h -- deep-zoom views with bilinear approximation (include/mbk.h, "Deep-zoom views with bilinear
// approximation"): the table builder (host), the kernel, and the one-pixel host twin the CPU tests read.
//
// While a pixel's offset dz is tiny against the reference orbit, dz -> 2 Z_m dz + dz^2 + dc is linear in (dz, dc) to working
// precision, and 2^l such steps collapse into dz -> A dz + B dc.  (A, B) and the radius r below which the map may be used
// are merged pairwise over the orbit into levels l = 0 .. ; entry j of level l covers the 2^l steps that start at
// m = 1 + j 2^l.  The kernel has deep_view_kernel's shape (mbk_deep.h) with one more branch per step: the lane takes the highest
// level its (dz, m, i) allows, or the plain step, and the z / bailout / rebase tail is common to both.  The orbit entries and
// level 0's rc come from a BlaCursor (mbk_deep_cursor.h).
//
// Memory: the rc values (r / sqrt 2, compared with max(|dz.r|, |dz.i|)) live in their own array, so probing the levels
// costs 8-byte loads only; (A, B) is one 32-byte entry, loaded once the level is chosen.  Level 0's rc rides one step ahead
// of its use, as the orbit entries do (the cursor's `rn`, `pre`), so a step that cannot skip pays no load latency for having
// asked.  After the first rebase the lanes of a wave hold different m: skip and plain step are the two sides of a divergent
// branch, and no wave-uniform value is taken from a lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mbk_deep.h"

namespace mbk {

static const double kBlaEps = 0x1p-40;                   // the contract's eps (mbk.h: looser values fail the truth tests)
static const double kBlaHalfSqrt2 = 0.7071067811865476;  // rc = fl(r * this)
static const uint32_t kBlaMaxLevels = 32;

// The table on the host: level l holds n[l] = (M - 1) >> l entries from off[l] on.
struct BlaTable {
    uint32_t levels = 0;
    uint32_t off[kBlaMaxLevels + 1] = {};
    std::vector<double> rc;     // per entry
    std::vector<double> ab;     // (A_r, A_i, B_r, B_i) per entry
    uint32_t count(uint32_t l) const { return off[l + 1] - off[l]; }
};

inline uint32_t bla_levels(uint32_t M)
{
    uint32_t levels = 0;
    if (M >= 2u)
        while (levels < kBlaMaxLevels && ((M - 1u) >> levels) >= 1u) ++levels;
    return levels;
}

// the entries of all levels together: level l holds (M - 1) >> l
inline uint64_t bla_entries(uint32_t M)
{
    uint64_t total = 0;
    for (uint32_t l = 0, n = bla_levels(M); l < n; ++l) total += (M - 1u) >> l;
    return total;
}

inline double bla_norm(double r, double i)
{
    const double a = r * r, b = i * i;
    return std::sqrt(a + b);
}

// `orbit` is DeepOrbit::table ((Zr, Zi, 2 Zr, 2 Zi) per entry, entries 0 .. M).  Every operation is rounded on its own (the
// translation unit is compiled -ffp-contract=off); tests/deep_bla_model.py (build) restates this in numpy.
inline void build_bla_table(const std::vector<double> &orbit, uint32_t M, double dcmax, BlaTable *out)
{
    BlaTable &t = *out;
    t = BlaTable();
    t.levels = bla_levels(M);
    uint64_t total = 0;
    for (uint32_t l = 0; l < t.levels; ++l) {
        t.off[l] = (uint32_t)total;
        total += (M - 1u) >> l;
    }
    t.off[t.levels] = (uint32_t)total;
    if (!t.levels) return;
    t.rc.resize(total);
    t.ab.resize(4 * total);
    std::vector<double> r(total);
    for (uint32_t j = 0; j < M - 1u; ++j) {
        const double ar = orbit[4 * (size_t)(j + 1u) + 2], ai = orbit[4 * (size_t)(j + 1u) + 3];
        double *e = &t.ab[4 * (size_t)j];
        e[0] = ar;
        e[1] = ai;
        e[2] = 1.0;
        e[3] = 0.0;
        r[j] = kBlaEps * bla_norm(ar, ai);
        t.rc[j] = r[j] * kBlaHalfSqrt2;
    }
    for (uint32_t l = 0; l + 1u < t.levels; ++l)
        for (uint32_t j = 0; j < t.count(l + 1u); ++j) {
            const size_t ix = (size_t)t.off[l] + 2u * j, iy = ix + 1u, io = (size_t)t.off[l + 1u] + j;
            const double *x = &t.ab[4 * ix], *y = &t.ab[4 * iy];
            const double Ar = y[0] * x[0] - y[1] * x[1];
            const double Ai = y[0] * x[1] + y[1] * x[0];
            const double Br = (y[0] * x[2] - y[1] * x[3]) + y[2];
            const double Bi = (y[0] * x[3] + y[1] * x[2]) + y[3];
            const double ax = bla_norm(x[0], x[1]), bx = bla_norm(x[2], x[3]);
            const double q = (r[iy] - bx * dcmax) / ax;
            const bool ok = ax != 0.0 && std::isfinite(Ar) && std::isfinite(Ai) && std::isfinite(Br) && std::isfinite(Bi) &&
                            std::isfinite(q);
            double ro = 0.0;
            if (ok) {
                ro = q > 0.0 ? q : 0.0;
                if (r[ix] < ro) ro = r[ix];
            }
            double *e = &t.ab[4 * io];
            e[0] = Ar;
            e[1] = Ai;
            e[2] = Br;
            e[3] = Bi;
            r[io] = ro;
            t.rc[io] = ro * kBlaHalfSqrt2;
        }
}

// ---- the step, shared by the kernel and the host twin ---------------------------------------------------------------------

// The highest level a pixel at orbit index m >= 1 may take with i the index of the step about to run and
// ad = max(|dz.r|, |dz.i|), GIVEN that level 0 passed (ad < rc of level 0 at m).  Every condition is monotone in the level,
// so the search goes upward and stops at the first failure.  Reads rc[off[t] + j] only for j < n_t.
__host__ __device__ inline uint32_t bla_climb(const double *rc, const uint32_t *off, uint32_t levels, uint32_t M, uint32_t m,
                                              int64_t i, int64_t mrd, double ad)
{
    const uint32_t k = m - 1u;
    uint32_t l = 0;
    for (uint32_t t = 1; t < levels; ++t) {
        if (k & ((1u << t) - 1u)) break;
        const uint32_t j = k >> t;
        if (j >= ((M - 1u) >> t)) break;
        if (i + ((int64_t)1 << t) > mrd) break;
        if (!(ad < rc[off[t] + j])) break;
        l = t;
    }
    return l;
}

// dz = A dz + B dc
__host__ __device__ inline void bla_apply(double Ar, double Ai, double Br, double Bi, double dcr, double dci, double &dzr,
                                          double &dzi)
{
    const double xr = Ar * dzr, yr = Ai * dzi, xi = Ar * dzi, yi = Ai * dzr;
    const double ur = Br * dcr, vr = Bi * dci, ui = Br * dci, vi = Bi * dcr;
    dzr = (xr - yr) + (ur - vr);
    dzi = (xi + yi) + (ui + vi);
}

// max(|dz.r|, |dz.i|) < rc, false if either is a NaN
__host__ __device__ inline bool bla_within(double dzr, double dzi, double rc, double *ad)
{
    const double a = dzr < 0.0 ? -dzr : dzr, b = dzi < 0.0 ? -dzi : dzi;
    *ad = a > b ? a : b;
    return a < rc && b < rc;
}

struct DeepBlaArgs {
    DeepArgs v;                      // M >= 2: an orbit of length 1 has no table and takes deep_view_kernel
    const double *rc;                // off[levels] values
    const double4 *ab;               // (A_r, A_i, B_r, B_i), the same indexing
    uint32_t levels;
    uint32_t off[kBlaMaxLevels];     // level l starts at off[l]
};

// The escape loop of the sample at offset dc with the table's skips (M >= 2), as deep_escape is the plain one: written once for
// deep_bla_kernel and the refine kernel of an adaptive render (mbk_deep_adaptive.h).
__device__ __forceinline__ EscapeSample deep_bla_escape(const DeepBlaArgs &q, double dcr, double dci)
{
    const DeepArgs &p = q.v;
    double dzr = dcr, dzi = dci;
    BlaCursor<double4, double> c(p.orbit, p.z1, p.M, q.rc, 0.0);   // the radius is level 0's rc; 0 at m == 0
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        double ad;
        if (bla_within(dzr, dzi, c.r0, &ad)) {
            const uint32_t l = bla_climb(q.rc, q.off, q.levels, c.M, c.m, i, p.mrd, ad);
            const double4 e = q.ab[q.off[l] + ((c.m - 1u) >> l)];
            bla_apply(e.x, e.y, e.z, e.w, dcr, dci, dzr, dzi);
            c.skip(l);
            i += (int32_t)((1u << l) - 1u);            // < mrd: the level was taken with i + 2^l <= mrd
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
    return EscapeSample{count, mag};
}

__global__ __launch_bounds__(64) void deep_bla_kernel(DeepBlaArgs q)
{
    const DeepArgs &p = q.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const EscapeSample e = deep_bla_escape(q, px.dcr, px.dci);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = e.count;
    if (p.bytes) p.bytes[o] = quantise(e.count, p.mrd, p.quant_wide, p.quant_rcp);
    if (p.smooth) p.smooth[o] = smooth_value(e.count, e.mag);
}

// One pixel on the host, from the functions the kernel uses: the count, |z|^2 at the escaping step, and the number of steps
// executed (a skip is one).  `orbit` as for build_bla_table; with no table (M <= 1) this is the plain rule.
inline void bla_count_host(const std::vector<double> &orbit, uint32_t M, const BlaTable &t, double dcr, double dci, int64_t mrd,
                           int32_t *count, double *mag, uint64_t *steps)
{
    const double *Z = orbit.data();
    double dzr, dzi, zr, zi;
    uint32_t m = deep_start(Z[4], Z[5], M, dcr, dci, dzr, dzi, zr, zi);
    *count = 0;
    *mag = 0.0;
    *steps = 0;
    for (int64_t i = 1; i < mrd; ++i) {
        ++*steps;
        double ad;
        if (t.levels && m >= 1u && bla_within(dzr, dzi, t.rc[m - 1u], &ad)) {
            const uint32_t l = bla_climb(t.rc.data(), t.off, t.levels, M, m, i, mrd, ad);
            const double *e = &t.ab[4 * ((size_t)t.off[l] + ((m - 1u) >> l))];
            bla_apply(e[0], e[1], e[2], e[3], dcr, dci, dzr, dzi);
            m += 1u << l;
            i += ((int64_t)1 << l) - 1;
        } else {
            deep_plain_step(Z[4 * (size_t)m + 2], Z[4 * (size_t)m + 3], dcr, dci, dzr, dzi);
            ++m;
        }
        zr = Z[4 * (size_t)m] + dzr;
        zi = Z[4 * (size_t)m + 1] + dzi;
        const double mg = zr * zr + zi * zi;
        if (mg >= 4.0) {
            *count = (int32_t)i;
            *mag = mg;
            return;
        }
        if (deep_rebase(mg, dzr, dzi) || m == M) {
            dzr = zr;
            dzi = zi;
            m = 0u;
        }
    }
}

}  // namespace mbk
