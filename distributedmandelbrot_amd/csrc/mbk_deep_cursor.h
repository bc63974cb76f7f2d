// mbk_deep_cursor.h -- what the deep kernels of both arithmetics share (mbk_deep*.h): a lane's pixel, and the cursor that
// walks a lane along the reference orbit.
//
// The cursor owns the orbit index m and the three table entries a step works from -- m (`cur`: the step's 2 Z_m), m + 1 (`nz`:
// the entry the step lands on, Z_{m+1}) and m + 2 (`pre`, loaded one step ahead so that its L1/L2 latency hides behind a
// step's dependent fp64 operations) -- and with them every clamp of the table's end.  One step of a kernel is
//     its own step from c.cur;  c.step()               or, with a table,  its own skip of 2^l;  c.skip(l)
//     z = c.nz + dz;  the bailout test
//     c.last() or the arithmetic's rebase test:  dz = z;  c.rebased()            otherwise  c.advanced()
//     c.prefetch()
// Between step() / skip() and rebased() / advanced(), m already names the entry in `nz`.  Entry 1, the state right after a
// rebase, comes with the kernel's arguments; entry 0 is zero and is never loaded.
//
// BlaCursor adds level 0's radius at m and at m + 1 (the second rides a step ahead, as `pre` does); the kernels without a table
// do not carry the pair.  Everything is __forceinline__ and lives in a kernel's local struct whose address never escapes, so
// all of it stays in registers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mbk_deep_orbit.h"

namespace mbk {

// ---- a lane's pixel ----

struct DeepPixel {
    uint32_t lc, lr;     // column and row within the window
    double dcr, dci;     // the pixel's offset from the view's centre (in units of 2^exp2 for a wide view)
    bool inside;         // false: the lane is past the window's edge and has nothing to do
};

// The offset of pixel (lc, lr) of the window: dc = fl(fl(k - (W-1)/2) * s); the subtraction is exact (|k| < 2^32, a half-integer
// at most).  Args: DeepArgs or DeepWideArgs.
template <typename Args>
__device__ __forceinline__ void deep_offset(const Args &p, uint32_t lc, uint32_t lr, double &dcr, double &dci)
{
    dcr = ((double)(p.col0 + lc) - p.half_r) * p.step_r;
    dci = ((double)(p.row0 + lr) - p.half_i) * p.step_i;
}

// One lane per pixel, one 8x8 block per single-wave workgroup, image order.
template <typename Args>
__device__ __forceinline__ DeepPixel deep_pixel(const Args &p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t by = blockIdx.x / p.blocks_x, bx = blockIdx.x - by * p.blocks_x;
    DeepPixel px;
    px.lc = bx * 8u + (lane & 7u);
    px.lr = by * 8u + (lane >> 3);
    px.inside = px.lc < p.ncols && px.lr < p.nrows;
    deep_offset(p, px.lc, px.lr, px.dcr, px.dci);
    return px;
}

// ---- the cursor ----

// What a step reads of entry m: 2 Z_m of a double4 (Z_m itself goes unread, and a copy of the whole vector would ride through
// the loop), all of a WideEntry.  Entry 0 is zero.
__device__ __forceinline__ void orbit_entry_current(double4 &cur, const double4 &e)
{
    cur.z = e.z;
    cur.w = e.w;
}
__device__ __forceinline__ void orbit_entry_current(WideEntry &cur, const WideEntry &e) { cur = e; }
__device__ __forceinline__ void orbit_entry_zero(double4 &cur) { cur.z = cur.w = 0.0; }
__device__ __forceinline__ void orbit_entry_zero(WideEntry &cur)
{
    cur.xr = cur.xi = 0.0;
    cur.xe = kWideZeroExp;
}

// How the cursor takes an entry from the table: a double4 as a value, a WideEntry by reference, so that the copy into `pre` goes
// straight from the table.  Each is the form in which that arithmetic's loops keep the parent's timing: by reference the
// binary64 loops, and by value the wide ones, come out measurably slower (profiles/deep_shared/README.md).
__device__ __forceinline__ double4 orbit_entry_load(const double4 *e) { return *e; }
__device__ __forceinline__ const WideEntry &orbit_entry_load(const WideEntry *e) { return *e; }

// Entry: double4 (mbk_deep.h) or WideEntry (mbk_deep_wide.h)
template <typename Entry>
struct OrbitCursor {
    const Entry *orbit;   // entries 0 .. M
    const Entry &z1;      // entry 1, in the kernel's arguments
    const uint32_t M;
    uint32_t m;
    Entry cur, nz, pre;   // entries m (what a step reads of it: orbit_entry_current), m + 1, m + 2

    // entry k, clamped to the table's end: the clamped value is loaded and never used (m == M rebases)
    __device__ __forceinline__ decltype(auto) at(uint32_t k) const { return orbit_entry_load(orbit + (k < M ? k : M)); }

    // m0 from deep_start / wide_start: 1, or 0 for an orbit of length 1, which has no Z_2 and starts rebased.  Keep z1 a
    // reference and keep this order (entry 2 through the clamp first, then the rebase): with z1 copied into the struct, or entry
    // 2 loaded on one side of a branch only, the compiler merges the two copies through a pointer and the struct goes to scratch.
    __device__ __forceinline__ OrbitCursor(const Entry *table, const Entry &entry1, uint32_t length, uint32_t m0)
        : orbit(table), z1(entry1), M(length)
    {
        m = 1u;
        orbit_entry_current(cur, z1);
        nz = at(2u);   // (an orbit of length 1: the clamp reads Z_1)
        if (m0 == 0u) rebased();
        prefetch();
    }
    __device__ __forceinline__ void step() { ++m; }
    // after a skip of 2^l steps: m <= M (entry j of level l ends at 1 + (j + 1) 2^l <= 1 + (M - 1))
    __device__ __forceinline__ void skip(uint32_t l)
    {
        m += 1u << l;
        nz = orbit[m];
        pre = at(m + 1u);
    }
    __device__ __forceinline__ bool last() const { return m == M; }
    // the pixel's own z has become its offset from Z_0 = 0
    __device__ __forceinline__ void rebased()
    {
        m = 0u;
        orbit_entry_zero(cur);
        nz = z1;
    }
    __device__ __forceinline__ void advanced()
    {
        orbit_entry_current(cur, nz);
        nz = pre;
    }
    __device__ __forceinline__ void prefetch() { pre = at(m + 2u); }
};

// The cursor of a kernel that takes bilinear-approximation skips (M >= 2: a shorter orbit has no table).  R: the type of level
// 0's radii -- double (mbk_deep_bla.h: rc) or int32_t (mbk_deep_wide_bla.h: ke).
template <typename Entry, typename R>
struct BlaCursor : OrbitCursor<Entry> {
    const R *radii;   // level 0: M - 1 values, the radius at orbit index k is radii[k - 1]
    const R none;     // the radius nothing passes: m == 0 has no entry and takes the plain step
    R r0, rn;         // the radius at m and at m + 1

    // the radius at orbit index k + 1, clamped to the level's end: the clamped value is loaded and never used (m == M rebases)
    __device__ __forceinline__ R radius(uint32_t k) const { return radii[k < this->M - 1u ? k : this->M - 2u]; }

    __device__ __forceinline__ BlaCursor(const Entry *table, const Entry &entry1, uint32_t length, const R *level0, R never)
        : OrbitCursor<Entry>(table, entry1, length, 1u), radii(level0), none(never)
    {
        r0 = radii[0];
        rn = radius(1u);
    }
    __device__ __forceinline__ void skip(uint32_t l)
    {
        OrbitCursor<Entry>::skip(l);
        rn = radius(this->m - 1u);   // level 0 at the new m
    }
    __device__ __forceinline__ void rebased()
    {
        OrbitCursor<Entry>::rebased();
        r0 = none;
    }
    __device__ __forceinline__ void advanced()
    {
        OrbitCursor<Entry>::advanced();
        r0 = rn;
    }
    __device__ __forceinline__ void prefetch()
    {
        OrbitCursor<Entry>::prefetch();
        rn = radius(this->m);
    }
};

}  // namespace mbk
