// mbk_deep_wide_bla.h -- extended-range deep views with bilinear approximation (include/mbk.h, "Extended-range deep views
// with bilinear approximation"): the table builder (host), the kernel, and the one-pixel host twin the CPU tests read.
//
// The idea is mbk_deep_bla.h's -- 2^l linear steps dz -> 2 Z_m dz + dc collapse into dz -> A dz + B dc, merged pairwise over
// the orbit -- in the number format of mbk_deep_wide.h: A and B are binary64 mantissa pairs with one int32 exponent each, the
// radius a mantissa with an exponent.  So |A|, which grows like 4^(2^l), has no binary64 ceiling, and a radius far below
// 1e-308 is as good as any other.  The radius test is an integer compare: per entry one int32 ke, the largest power of two
// not above r / sqrt 2, against the exponent q of the pixel's dz = w 2^q (max(|w_r|, |w_i|) < 1, so q <= ke puts both
// components below r / sqrt 2).
//
// Memory: the ke values live in their own array, so probing the levels costs 4-byte loads only; (A, B) is one 48-byte
// entry, loaded once the level is chosen.  Level 0's ke rides one step ahead of its use, as the orbit entries do (`rn`,
// `pre` of the BlaCursor, mbk_deep_cursor.h).  The kernel has deep_wide_kernel's shape with one more branch per step: skip and
// plain step are the two sides of a divergent branch, the z / bailout / rebase tail is common to both, and no wave-uniform value
// is taken from a lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "mbk_deep_bla.h"
#include "mbk_deep_wide.h"

namespace mbk {

static const int32_t kWideBlaEpsExp = -40;          // eps = 2^-40, as the plain contract's (mbk.h: held to the truth again)
static const int32_t kWideBlaMaxExp = 1 << 20;      // a live A, B or r has no exponent beyond this in magnitude

// (A, B) of one entry: A = (ar, ai) 2^ae, B = (br, bi) 2^be; a dead entry is all zeros with both exponents kWideZeroExp
struct alignas(16) WideBlaEntry {
    double ar, ai, br, bi;
    int32_t ae, be;
    int32_t pad[2];
};

// The table on the host: level l holds n[l] = (M - 1) >> l entries from off[l] on.
struct WideBlaTable {
    uint32_t levels = 0;
    uint32_t off[kBlaMaxLevels + 1] = {};
    std::vector<int32_t> ke;            // per entry
    std::vector<WideBlaEntry> ab;       // per entry
    uint32_t count(uint32_t l) const { return off[l + 1] - off[l]; }
};

// a non-negative real f 2^e with f in [0.5, 1), or (0, kWideZeroExp)
struct WideReal {
    double f;
    int32_t e;
};

inline WideReal wide_real(double v, int32_t e)
{
    if (!(v > 0.0)) return WideReal{0.0, kWideZeroExp};
    const int32_t s = wide_exp(v);
    return WideReal{std::ldexp(v, -s), e + s};
}

// |(r, i) 2^e|: the mantissa is fl(sqrt(fl(fl(r^2) + fl(i^2))))
inline WideReal wide_abs(double r, double i, int32_t e)
{
    const double a = r * r, b = i * i;
    const double s = a + b;
    return wide_real(std::sqrt(s), e);
}

inline bool wide_less(const WideReal &a, const WideReal &b) { return a.e != b.e ? a.e < b.e : a.f < b.f; }

// dcmax of the contract: fl(|dcm_r(column 0)| + |dcm_i(row 0)|) 2^exp2, normalised
inline WideReal wide_dcmax(double dcr0, double dci0, int32_t exp2)
{
    const double a = std::fabs(dcr0), b = std::fabs(dci0);
    const double s = a + b;
    return wide_real(s, exp2);
}

// r -> ke: the largest integer with 2^ke <= fl(f 0.7071067811865476) 2^e
inline int32_t wide_bla_ke(const WideReal &r)
{
    if (r.f == 0.0) return kWideZeroExp;
    const double c = r.f * kBlaHalfSqrt2;
    return r.e + wide_exp(c) - 1;
}

inline bool wide_bla_exp_ok(int32_t e) { return e == kWideZeroExp || (e <= kWideBlaMaxExp && e >= -kWideBlaMaxExp); }

// `orbit` is DeepOrbit::wide (entries 0 .. M).  Every operation is rounded on its own (the translation unit is compiled
// -ffp-contract=off); tests/deep_wide_bla_model.py (build) restates this in numpy.
inline void build_wide_bla_table(const std::vector<WideEntry> &orbit, uint32_t M, const WideReal &dcmax, WideBlaTable *out)
{
    WideBlaTable &t = *out;
    t = WideBlaTable();
    t.levels = bla_levels(M);
    uint64_t total = 0;
    for (uint32_t l = 0; l < t.levels; ++l) {
        t.off[l] = (uint32_t)total;
        total += (M - 1u) >> l;
    }
    t.off[t.levels] = (uint32_t)total;
    if (!t.levels) return;
    const WideBlaEntry dead = {0.0, 0.0, 0.0, 0.0, kWideZeroExp, kWideZeroExp, {0, 0}};
    t.ke.resize(total);
    t.ab.resize(total);
    std::vector<WideReal> r(total);
    for (uint32_t j = 0; j < M - 1u; ++j) {
        const WideEntry &z = orbit[j + 1u];
        WideReal a = wide_abs(z.xr, z.xi, z.xe == kWideZeroExp ? kWideZeroExp : z.xe + 1);
        if (a.f == 0.0) {
            t.ab[j] = dead;
            r[j] = WideReal{0.0, kWideZeroExp};
        } else {
            t.ab[j] = WideBlaEntry{z.xr, z.xi, 1.0, 0.0, z.xe + 1, 0, {0, 0}};
            wide_norm(1.0, 0.0, 0, t.ab[j].br, t.ab[j].bi, t.ab[j].be);
            r[j] = WideReal{a.f, a.e + kWideBlaEpsExp};
        }
        t.ke[j] = wide_bla_ke(r[j]);
    }
    for (uint32_t l = 0; l + 1u < t.levels; ++l)
        for (uint32_t j = 0; j < t.count(l + 1u); ++j) {
            const size_t ix = (size_t)t.off[l] + 2u * j, iy = ix + 1u, io = (size_t)t.off[l + 1u] + j;
            const WideBlaEntry &x = t.ab[ix], &y = t.ab[iy];
            WideBlaEntry o = dead;
            WideReal ro = {0.0, kWideZeroExp};
            if (r[ix].f != 0.0 && r[iy].f != 0.0) {
                // A = A_y A_x
                const double aa = y.ar * x.ar, ab = y.ai * x.ai, ac = y.ar * x.ai, ad = y.ai * x.ar;
                wide_norm(aa - ab, ac + ad, y.ae + x.ae, o.ar, o.ai, o.ae);
                // B = A_y B_x + B_y
                const double ba = y.ar * x.br, bb = y.ai * x.bi, bc = y.ar * x.bi, bd = y.ai * x.br;
                const double qr = ba - bb, qi = bc + bd;
                const int32_t qe = y.ae + x.be, h = wide_max(qe, y.be);
                const double sr = wide_sh(qr, qe - h) + wide_sh(y.br, y.be - h);
                const double si = wide_sh(qi, qe - h) + wide_sh(y.bi, y.be - h);
                wide_norm(sr, si, h, o.br, o.bi, o.be);
                // t = (r_y - |B_x| dcmax) / |A_x|
                const WideReal ax = wide_abs(x.ar, x.ai, x.ae), bx = wide_abs(x.br, x.bi, x.be);
                const double u = bx.f * dcmax.f;
                const int32_t ue = bx.e + dcmax.e, g = wide_max(r[iy].e, ue);
                const double d = wide_sh(r[iy].f, r[iy].e - g) - wide_sh(u, ue - g);
                if (ax.f != 0.0 && d > 0.0 && wide_bla_exp_ok(o.ae) && wide_bla_exp_ok(o.be)) {
                    const double v = d / ax.f;
                    ro = wide_real(v, g - ax.e);
                    if (wide_less(r[ix], ro)) ro = r[ix];
                    if (ro.e < -kWideBlaMaxExp) ro = WideReal{0.0, kWideZeroExp};
                }
                if (ro.f == 0.0) o = dead;
            }
            t.ab[io] = o;
            r[io] = ro;
            t.ke[io] = wide_bla_ke(ro);
        }
}

// ---- the step, shared by the kernel and the host twin ---------------------------------------------------------------------

// The entry of the highest level a pixel at orbit index m >= 1 may take with i the index of the step about to run and q the
// exponent of its dz, GIVEN that level 0 passed (q <= ke of level 0 at m).  Every condition is monotone in the level, so the
// search goes upward and stops at the first failure.  Reads ke[off[t] + j] only for j < n_t.  *level receives the level.
__host__ __device__ inline uint32_t wide_bla_climb(const int32_t *ke, const uint32_t *off, uint32_t levels, uint32_t M, uint32_t m,
                                                   int64_t i, int64_t mrd, int32_t q, uint32_t *level)
{
    const uint32_t k = m - 1u;
    uint32_t l = 0, at = k;
    for (uint32_t t = 1; t < levels; ++t) {
        if (k & ((1u << t) - 1u)) break;
        const uint32_t j = k >> t;
        if (j >= ((M - 1u) >> t)) break;
        if (i + ((int64_t)1 << t) > mrd) break;
        if (!(q <= ke[off[t] + j])) break;
        l = t;
        at = off[t] + j;
    }
    *level = l;
    return at;
}

// (w, q) = norm(A w 2^(ae + q) + B dcm 2^(be + exp2))
__host__ __device__ inline void wide_bla_apply(double ar, double ai, int32_t ae, double br, double bi, int32_t be, double dcr,
                                               double dci, int32_t exp2, double &wr, double &wi, int32_t &q)
{
    const double xr = ar * wr, yr = ai * wi, xi = ar * wi, yi = ai * wr;
    const double ur = br * dcr, vr = bi * dci, ui = br * dci, vi = bi * dcr;
    const double p1r = xr - yr, p1i = xi + yi;
    const double p2r = ur - vr, p2i = ui + vi;
    const int32_t e1 = ae + q, e2 = be + exp2, h = wide_max(e1, e2);
    const double Nr = wide_sh(p1r, e1 - h) + wide_sh(p2r, e2 - h);
    const double Ni = wide_sh(p1i, e1 - h) + wide_sh(p2i, e2 - h);
    wide_norm(Nr, Ni, h, wr, wi, q);
}

// the radius test: a zero dz (q = kWideZeroExp) and a dead entry (ke = kWideZeroExp) never pass
__host__ __device__ inline bool wide_bla_within(int32_t q, int32_t ke) { return q > kWideZeroExp && q <= ke; }

struct DeepWideBlaArgs {
    DeepWideArgs v;                  // M >= 2: an orbit of length 1 has no table and takes deep_wide_kernel
    const int32_t *ke;               // off[levels] values
    const WideBlaEntry *ab;          // the same indexing
    uint32_t levels;
    uint32_t off[kBlaMaxLevels];     // level l starts at off[l]
};

// The escape loop of the sample at offset dc 2^exp2 with the table's skips (M >= 2), as deep_wide_escape is the plain one:
// written once for deep_wide_bla_kernel and the refine kernel of an adaptive render (mbk_deep_wide_adaptive.h).
__device__ __forceinline__ EscapeSample deep_wide_bla_escape(const DeepWideBlaArgs &a, double dcr, double dci)
{
    const DeepWideArgs &p = a.v;
    const int32_t exp2 = p.exp2;
    double wr, wi;
    int32_t q;
    wide_norm(dcr, dci, exp2, wr, wi, q);
    BlaCursor<WideEntry, int32_t> c(p.orbit, p.z1, p.M, a.ke, kWideZeroExp);   // the radius is level 0's ke; kWideZeroExp at m == 0
    int32_t count = 0;
    double mag = 0.0;
    for (int32_t i = 1; i < p.mrd; ++i) {
        if (wide_bla_within(q, c.r0)) {
            uint32_t l;
            const uint32_t at = wide_bla_climb(a.ke, a.off, a.levels, c.M, c.m, i, p.mrd, q, &l);
            const WideBlaEntry e = a.ab[at];
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
    return EscapeSample{count, mag};
}

__global__ __launch_bounds__(64) void deep_wide_bla_kernel(DeepWideBlaArgs a)
{
    const DeepWideArgs &p = a.v;
    const DeepPixel px = deep_pixel(p);
    if (!px.inside) return;
    const EscapeSample e = deep_wide_bla_escape(a, px.dcr, px.dci);
    const size_t o = (size_t)px.lr * p.ncols + px.lc;
    if (p.counts) p.counts[o] = e.count;
    if (p.bytes) p.bytes[o] = quantise(e.count, p.mrd, p.quant_wide, p.quant_rcp);
    if (p.smooth) p.smooth[o] = smooth_value(e.count, e.mag);
}

// One pixel on the host, from the functions the kernel uses: the count, |z|^2 at the escaping step, and the number of steps
// executed (a skip is one).  With no table (M <= 1) this is the plain wide rule.
inline void wide_bla_count_host(const std::vector<WideEntry> &orbit, uint32_t M, const WideBlaTable &tb, double dcr, double dci,
                                int32_t exp2, int64_t mrd, int32_t *count, double *mag, uint64_t *steps)
{
    const WideEntry *Z = orbit.data();
    double wr, wi, zr, zi, mg;
    int32_t q, t;
    uint32_t m = wide_start(Z[1], M, dcr, dci, exp2, wr, wi, q, zr, zi, t, mg);
    *count = 0;
    *mag = 0.0;
    *steps = 0;
    for (int64_t i = 1; i < mrd; ++i) {
        ++*steps;
        if (tb.levels && m >= 1u && wide_bla_within(q, tb.ke[m - 1u])) {
            uint32_t l;
            const uint32_t at = wide_bla_climb(tb.ke.data(), tb.off, tb.levels, M, m, i, mrd, q, &l);
            const WideBlaEntry &e = tb.ab[at];
            wide_bla_apply(e.ar, e.ai, e.ae, e.br, e.bi, e.be, dcr, dci, exp2, wr, wi, q);
            m += 1u << l;
            i += ((int64_t)1 << l) - 1;
        } else {
            wide_step(Z[m].xr, Z[m].xi, Z[m].xe, dcr, dci, exp2, wr, wi, q);
            ++m;
        }
        wide_z(Z[m].xr, Z[m].xi, Z[m].xe, wr, wi, q, zr, zi, t, mg);
        const double mgs = wide_mag(mg, t);
        if (mgs >= 4.0) {
            *count = (int32_t)i;
            *mag = mgs;
            return;
        }
        if (wide_rebase(mg, wr, wi, q, t) || m == M) {
            wide_norm(zr, zi, t, wr, wi, q);
            m = 0u;
        }
    }
}

}  // namespace mbk
