// mbk_loops.inc -- the hand-scheduled escape loops, written once and instantiated per arithmetic type.
// #include'd by mbk_kernels.h twice: MBK_T = double / MBK_F = "f64" (the reference's arithmetic) and
// MBK_T = float / MBK_F = "f32" (BASELINE cfg4's fp32 variant -- a new feature, not in the reference).
// The two instantiations are overloads on the coordinate type.  No include guard on purpose.
#ifndef MBK_T
#error "define MBK_T and MBK_F before including mbk_loops.inc"
#endif
// ---------------------------------------------------------------------------------------------
// Kernel "asm": same pixel mapping as "simple", but the escape loop is a hand-scheduled gfx950
// instruction stream.  Why: the compiler's structured-CFG loop spends ~14 SALU instructions and 3
// branches per iteration on EXEC bookkeeping; a CU has ONE scalar pipe for its four SIMDs, so at 8
// waves/SIMD the compiler loop is scalar-issue bound (measured 1.7 T pixel-iter/s, ~72 cycles per
// wave-iteration) instead of fp64-VALU bound (7 x 4 cycles).  This loop issues, per iteration,
// 7 fp64 VALU + 1 v_cmp + 1 branch, plus 3 SALU per FOUR iterations:
//   * the iteration counter lives in an SGPR (uniform) and is bumped once per 4 unrolled steps;
//   * "some lane escaped" is the rare path: `s_cbranch_vccnz` jumps out of line, where the escaped
//     lanes record the step index and leave EXEC; when EXEC empties the wave leaves the loop at
//     once (the wavefront-level early exit);
//   * v_cmp_le_f64 vcc, 4.0, m implements `m >= 4` with IEEE semantics (false for NaN).
// kFmaDouble = false swaps fma(2, zr*zi, ci) for the literal (zr+zr)*zi + ci (8 fp64 ops).
// ---------------------------------------------------------------------------------------------
#define MBK_STEP_HEAD_FMA                                  \
    "v_add_" MBK_F " %[t], %[a], -%[b]\n"                        \
    "v_mul_" MBK_F " %[p], %[zr], %[zi]\n"                       \
    "v_add_" MBK_F " %[zr], %[t], %[cr]\n"                       \
    "v_fma_" MBK_F " %[zi], %[p], 2.0, %[ci]\n"
#define MBK_STEP_HEAD_SAFE                                 \
    "v_add_" MBK_F " %[t], %[a], -%[b]\n"                        \
    "v_add_" MBK_F " %[p], %[zr], %[zr]\n"                       \
    "v_mul_" MBK_F " %[p], %[p], %[zi]\n"                        \
    "v_add_" MBK_F " %[zr], %[t], %[cr]\n"                       \
    "v_add_" MBK_F " %[zi], %[p], %[ci]\n"
#define MBK_STEP_TAIL(ID)                                  \
    "v_mul_" MBK_F " %[a], %[zr], %[zr]\n"                       \
    "v_mul_" MBK_F " %[b], %[zi], %[zi]\n"                       \
    "v_add_" MBK_F " %[m], %[a], %[b]\n"                         \
    "v_cmp_le_" MBK_F " vcc, 4.0, %[m]\n"                        \
    "s_cbranch_vccnz .Lesc" ID "_%=\n"                     \
    ".Lcont" ID "_%=:\n"
// out-of-line: lanes in VCC escaped at step N+INC
#define MBK_ESCAPE(ID, INC)                                \
    ".Lesc" ID "_%=:\n"                                    \
    "s_add_u32 %[k], %[n], " INC "\n"                      \
    "s_and_saveexec_b64 %[tmp], vcc\n"                     \
    "v_mov_b32 %[cnt], %[k]\n"                             \
    "s_andn2_b64 exec, %[tmp], vcc\n"                      \
    "s_cbranch_scc1 .Lcont" ID "_%=\n"                     \
    "s_branch .Ldone_%=\n"
#define MBK_LOOP_ASM(HEAD)                                 \
    "s_mov_b64 %[save], exec\n"                            \
    "s_mov_b32 %[n], %[n0]\n"                              \
    "s_cmp_ge_u32 %[n], %[limit4]\n"                       \
    "s_cbranch_scc1 .Ltail_%=\n"                           \
    ".Lmain_%=:\n"                                         \
    HEAD MBK_STEP_TAIL("1") HEAD MBK_STEP_TAIL("2")        \
    HEAD MBK_STEP_TAIL("3") HEAD MBK_STEP_TAIL("4")        \
    "s_add_u32 %[n], %[n], 4\n"                            \
    "s_cmp_lt_u32 %[n], %[limit4]\n"                       \
    "s_cbranch_scc1 .Lmain_%=\n"                           \
    ".Ltail_%=:\n"                                         \
    "s_cmp_ge_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Ldone_%=\n"                           \
    ".Ltloop_%=:\n"                                        \
    HEAD MBK_STEP_TAIL("T")                                \
    "s_add_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lt_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Ltloop_%=\n"                          \
    "s_branch .Ldone_%=\n"                                 \
    MBK_ESCAPE("1", "1") MBK_ESCAPE("2", "2") MBK_ESCAPE("3", "3") MBK_ESCAPE("4", "4")  \
    MBK_ESCAPE("T", "1")                                   \
    ".Ldone_%=:\n"                                         \
    "s_mov_b64 exec, %[save]\n"

// Per-step loop: runs steps n0+1 .. stop on the state (zr, zi, a = zr^2, b = zi^2); lanes that escape
// get cnt = step index and leave; survivors keep cnt unchanged and their state advanced to `stop`.
template <bool kFmaDouble>
__device__ __forceinline__ void escape_steps_asm(MBK_T cr, MBK_T ci, MBK_T &zr, MBK_T &zi, MBK_T &a,
                                                 MBK_T &b, MBK_T &m, int32_t &cnt, uint32_t n0, uint32_t stop)
{
    // m: |z|^2 of the last step each lane executed; an escaped lane leaves EXEC at once, so for it m
    // stays the value that tripped the test (used by the smooth-colouring epilogue)
    MBK_T t, p;
    const uint32_t total = stop;                         // uniform
    const uint32_t limit4 = n0 + ((stop - n0) & ~3u);    // whole 4-step trips
    uint32_t n, k;
    unsigned long long save, tmp;
    if (kFmaDouble) {
        asm volatile(MBK_LOOP_ASM(MBK_STEP_HEAD_FMA)
                     : [zr] "+&v"(zr), [zi] "+&v"(zi), [a] "+&v"(a), [b] "+&v"(b), [cnt] "+&v"(cnt),
                       [m] "+&v"(m), [t] "=&v"(t), [p] "=&v"(p), [n] "=&s"(n), [k] "=&s"(k),
                       [save] "=&s"(save), [tmp] "=&s"(tmp)
                     : [cr] "v"(cr), [ci] "v"(ci), [total] "s"(total), [limit4] "s"(limit4), [n0] "s"(n0)
                     : "vcc", "scc");
    } else {
        asm volatile(MBK_LOOP_ASM(MBK_STEP_HEAD_SAFE)
                     : [zr] "+&v"(zr), [zi] "+&v"(zi), [a] "+&v"(a), [b] "+&v"(b), [cnt] "+&v"(cnt),
                       [m] "+&v"(m), [t] "=&v"(t), [p] "=&v"(p), [n] "=&s"(n), [k] "=&s"(k),
                       [save] "=&s"(save), [tmp] "=&s"(tmp)
                     : [cr] "v"(cr), [ci] "v"(ci), [total] "s"(total), [limit4] "s"(limit4), [n0] "s"(n0)
                     : "vcc", "scc");
    }
}

template <bool kFmaDouble>
__device__ __forceinline__ int32_t escape_count_asm(MBK_T cr, MBK_T ci, int32_t mrd, MBK_T *m_out = nullptr)
{
    MBK_T zr = cr, zi = ci;
    MBK_T a = zr * zr, b = zi * zi, m = 0;
    int32_t cnt = 0;
    escape_steps_asm<kFmaDouble>(cr, ci, zr, zi, a, b, m, cnt, 0u, mrd > 1 ? (uint32_t)mrd - 1u : 0u);
    if (m_out) *m_out = m;
    return cnt;
}

// ---------------------------------------------------------------------------------------------
// Grouped bailout test ("group" loop).  The bailout compare costs a full fp64 issue slot (v_cmp writes
// an SGPR pair: 4.4 cycles, measured) and needs m = a + b, another slot: 2 of the 8 slots of a step.
// Once |z|^2 >= 4 the orbit cannot come back below 4 (for |c| <= 2 - 1e-9:
// |z'| >= |z|^2 - |c| >= 2 with margin over rounding; for |c| >= 2 + 1e-9 it escapes at step 1 and
// |z| >= |c| grows; it ends in inf and then NaN), so it is enough to test after every G = 4 steps
// with a NaN-inclusive compare (v_cmp_ngt_f64 vcc, 4.0, m == !(4 > m)), and to find the exact step
// afterwards: the four unchecked steps run on a scratch register set and leave the group's start
// state intact, so the lanes that tripped the test REPLAY those four steps with the exact per-step
// IEEE test (v_cmp_le_f64 4.0 <= m) and record the first hit -- since round 3 not on the spot but once
// per wave, after its loop ("deferred replay" below).  Result: 6 fp64 VALU per step + 2 per
// group = 6.5 slots per step instead of 8, bit-identical counts.
// Waves that contain a pixel with | |c|^2 - 4 | < 1e-9 (the one place where "stays >= 4" could be
// spoiled by rounding) take the per-step loop instead (tile_asm_kernel's `risky` branch).
// Register sets: A = (zr, zi, a, b) and B = (zr2, zi2, a2, b2) alternate as group start/end; T is the
// scratch set.  One loop trip = group A->B + group B->A = 8 steps.
// ---------------------------------------------------------------------------------------------
#define MBK_G_STEP(ZRS, ZIS, AS, BS, ZRD, ZID, AD, BD)     \
    "v_add_" MBK_F " %[t], " AS ", -" BS "\n"                    \
    "v_mul_" MBK_F " %[p], " ZRS ", " ZIS "\n"                   \
    "v_add_" MBK_F " " ZRD ", %[t], %[cr]\n"                     \
    "v_fma_" MBK_F " " ZID ", %[p], 2.0, %[ci]\n"                \
    "v_mul_" MBK_F " " AD ", " ZRD ", " ZRD "\n"                 \
    "v_mul_" MBK_F " " BD ", " ZID ", " ZID "\n"
#define MBK_G_A2T MBK_G_STEP("%[zr]", "%[zi]", "%[a]", "%[b]", "%[zrt]", "%[zit]", "%[at]", "%[bt]")
#define MBK_G_B2T MBK_G_STEP("%[zr2]", "%[zi2]", "%[a2]", "%[b2]", "%[zrt]", "%[zit]", "%[at]", "%[bt]")
#define MBK_G_T2T MBK_G_STEP("%[zrt]", "%[zit]", "%[at]", "%[bt]", "%[zrt]", "%[zit]", "%[at]", "%[bt]")
#define MBK_G_T2A MBK_G_STEP("%[zrt]", "%[zit]", "%[at]", "%[bt]", "%[zr]", "%[zi]", "%[a]", "%[b]")
#define MBK_G_T2B MBK_G_STEP("%[zrt]", "%[zit]", "%[at]", "%[bt]", "%[zr2]", "%[zi2]", "%[a2]", "%[b2]")
// four unchecked steps (FIRST, T2T, T2T, LAST), then the NaN-inclusive group test on the end set
#define MBK_G_GROUP(FIRST, LAST, AD, BD, ID)               \
    FIRST MBK_G_T2T MBK_G_T2T LAST                         \
    "v_add_" MBK_F " %[m], " AD ", " BD "\n"                     \
    "v_cmp_ngt_" MBK_F " vcc, 4.0, %[m]\n"                       \
    "s_cbranch_vccnz .Lgrep" ID "_%=\n"                    \
    ".Lgcont" ID "_%=:\n"
// ---- deferred replay (round 3) ---------------------------------------------------------------------------
// Rounds 1-2 replayed a group on the spot: the lanes that tripped its test re-ran its G steps with the exact
// per-step test (9 issue slots per replayed step) while the rest of the wave waited -- once per GROUP in which some
// lane escaped, i.e. many times per boundary block (cfg2: 9.6 M of a launch's 311.9 M VALU instructions; with the
// cycle test, where the set's interior is cheap, 6 %).  But a lane that leaves EXEC is frozen: nothing writes its
// registers any more.  So a tripped lane now just LEAVES, with the clock of its group's start in cnt (bit 31 marks
// it pending) and its group-start state in register set A -- where it already is when the group started from set
// A; the second group of a trip starts from set B, whose four values are copied over first.  When the wave is
// done, ONE fix-up loop runs all pending lanes together, each from its own start state, through at most G exact
// steps (v_cmp_le 4.0 <= m, the reference's test; cnt counts up by one per step) and every lane drops out at its
// first hit: the same arithmetic from the same state as the on-the-spot replay, so the same escape index and the
// same |z|^2 in m.  A trip costs 1 (set A) or 5 (set B) VALU instructions instead of ~40-70, the fix-up 9 G once.
// A pending lane that finds no hit within G steps (impossible inside the coordinate bound: an inf is caught by the
// exact test at the step it appears, before any NaN) ends as 0, which is what the old scheme returned for it.
#define MBK_G_TRIP_A(ID, BASE)                             \
    ".Lgrep" ID "_%=:\n"                                   \
    "s_and_saveexec_b64 %[tmp], vcc\n"                     \
    "s_add_u32 %[k], %[n], " BASE "\n"                     \
    "s_or_b32 %[k], %[k], 0x80000000\n"                    \
    "v_mov_b32 %[cnt], %[k]\n"                             \
    "s_andn2_b64 exec, %[tmp], vcc\n"                      \
    "s_cbranch_scc1 .Lgcont" ID "_%=\n"                    \
    "s_branch .Lgdone_%=\n"
#define MBK_G_TRIP_B(ID, BASE)                             \
    ".Lgrep" ID "_%=:\n"                                   \
    "s_and_saveexec_b64 %[tmp], vcc\n"                     \
    "v_mov_" MBK_CYC_MOV " %[zr], %[zr2]\n"                \
    "v_mov_" MBK_CYC_MOV " %[zi], %[zi2]\n"                \
    "v_mov_" MBK_CYC_MOV " %[a], %[a2]\n"                  \
    "v_mov_" MBK_CYC_MOV " %[b], %[b2]\n"                  \
    "s_add_u32 %[k], %[n], " BASE "\n"                     \
    "s_or_b32 %[k], %[k], 0x80000000\n"                    \
    "v_mov_b32 %[cnt], %[k]\n"                             \
    "s_andn2_b64 exec, %[tmp], vcc\n"                      \
    "s_cbranch_scc1 .Lgcont" ID "_%=\n"                    \
    "s_branch .Lgdone_%=\n"
#define MBK_G_A2A MBK_G_STEP("%[zr]", "%[zi]", "%[a]", "%[b]", "%[zr]", "%[zi]", "%[a]", "%[b]")
// runs with EXEC = the asm block's entry mask (%[save]); leaves EXEC undefined (the caller restores it)
#define MBK_G_FIXUP(G)                                     \
    "v_cmp_gt_i32 vcc, 0, %[cnt]\n"                        \
    "v_cmp_ne_u32_e64 %[tmp2], -1, %[cnt]\n"   /* -1 = retired by the cycle test, not pending */ \
    "s_and_b64 vcc, vcc, %[tmp2]\n"                        \
    "s_cbranch_vccz .Lgfixed_%=\n"                         \
    "s_mov_b64 exec, vcc\n"                                \
    "v_and_b32 %[cnt], 0x7fffffff, %[cnt]\n"               \
    "s_mov_b32 %[k], " G "\n"                              \
    ".Lgfix_%=:\n"                                         \
    MBK_G_A2A                                              \
    "v_add_" MBK_F " %[m], %[a], %[b]\n"                   \
    "v_add_u32 %[cnt], 1, %[cnt]\n"                        \
    "v_cmp_le_" MBK_F " vcc, 4.0, %[m]\n"                  \
    "s_andn2_b64 exec, exec, vcc\n"                        \
    "s_cbranch_execz .Lgfixed_%=\n"                        \
    "s_sub_u32 %[k], %[k], 1\n"                            \
    "s_cmp_lg_u32 %[k], 0\n"                               \
    "s_cbranch_scc1 .Lgfix_%=\n"                           \
    "v_mov_b32 %[cnt], 0\n"                                \
    ".Lgfixed_%=:\n"
#define MBK_G_LOOP                                         \
    "s_mov_b64 %[save], exec\n"                            \
    "s_mov_b32 %[n], %[n0]\n"                              \
    "s_cmp_ge_u32 %[n], %[limit8]\n"                          \
    "s_cbranch_scc1 .Lgtail_%=\n"                          \
    ".Lgmain_%=:\n"                                        \
    MBK_G_GROUP(MBK_G_A2T, MBK_G_T2B, "%[a2]", "%[b2]", "1") \
    MBK_G_GROUP(MBK_G_B2T, MBK_G_T2A, "%[a]", "%[b]", "2")    \
    "s_add_u32 %[n], %[n], 8\n"                            \
    "s_cmp_lt_u32 %[n], %[limit8]\n"                       \
    "s_cbranch_scc1 .Lgmain_%=\n"                          \
    ".Lgtail_%=:\n"                                        \
    "s_cmp_ge_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgdone_%=\n"                          \
    ".Lgtloop_%=:\n"                                       \
    MBK_STEP_HEAD_FMA MBK_STEP_TAIL("GT")                  \
    "s_add_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lt_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgtloop_%=\n"                         \
    "s_branch .Lgdone_%=\n"                                \
    MBK_G_TRIP_A("1", "0")                                 \
    MBK_G_TRIP_B("2", "4")                                 \
    MBK_ESCAPE("GT", "1")                                  \
    ".Ldone_%=:\n"                                         \
    ".Lgdone_%=:\n"                                        \
    "s_mov_b64 exec, %[save]\n"                            \
    MBK_G_FIXUP("4")                                       \
    "s_mov_b64 exec, %[save]\n"

// ---- same scheme with 8 steps per group (6.25 slots per step; one trip = 16 steps) -------------
#define MBK_G_GROUP8(FIRST, LAST, AD, BD, ID)              \
    FIRST MBK_G_T2T MBK_G_T2T MBK_G_T2T MBK_G_T2T MBK_G_T2T MBK_G_T2T LAST \
    "v_add_" MBK_F " %[m], " AD ", " BD "\n"                     \
    "v_cmp_ngt_" MBK_F " vcc, 4.0, %[m]\n"                       \
    "s_cbranch_vccnz .Lgrep" ID "_%=\n"                    \
    ".Lgcont" ID "_%=:\n"
#define MBK_G_LOOP8X(INIT, CYC1, CYC2, OOL, FIX)                             \
    "s_mov_b64 %[save], exec\n"                            \
    "s_mov_b32 %[n], %[n0]\n"                              \
    INIT                                                   \
    "s_cmp_ge_u32 %[n], %[limit8]\n"                          \
    "s_cbranch_scc1 .Lgtail_%=\n"                          \
    ".Lgmain_%=:\n"                                        \
    MBK_G_GROUP8(MBK_G_A2T, MBK_G_T2B, "%[a2]", "%[b2]", "1") \
    CYC1                                                   \
    MBK_G_GROUP8(MBK_G_B2T, MBK_G_T2A, "%[a]", "%[b]", "2")   \
    CYC2                                                   \
    "s_add_u32 %[n], %[n], 16\n"                           \
    "s_cmp_lt_u32 %[n], %[limit8]\n"                       \
    "s_cbranch_scc1 .Lgmain_%=\n"                          \
    ".Lgtail_%=:\n"                                        \
    "s_cmp_ge_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgdone_%=\n"                          \
    ".Lgtloop_%=:\n"                                       \
    MBK_STEP_HEAD_FMA MBK_STEP_TAIL("GT")                  \
    "s_add_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lt_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgtloop_%=\n"                         \
    "s_branch .Lgdone_%=\n"                                \
    MBK_G_TRIP_A("1", "0")                                 \
    MBK_G_TRIP_B("2", "8")                                 \
    MBK_ESCAPE("GT", "1")                                  \
    OOL                                                    \
    ".Ldone_%=:\n"                                         \
    ".Lgdone_%=:\n"                                        \
    "s_mov_b64 exec, %[save]\n"                            \
    FIX                                                    \
    "s_mov_b64 exec, %[save]\n"
#define MBK_G_LOOP8 MBK_G_LOOP8X("", "", "", "", MBK_G_FIXUP("8"))
// (FIX = "": the lanes that tripped a group test stay pending -- cnt keeps bit 31 and the clock of the group's start, register
// set A the group's start state; nothing touches a lane that has left EXEC -- until the caller runs escape_fixup once for all
// the stretches it has run: block_pixel_spill, whose blocks run their steps in several stretches)
#define MBK_G_LOOP8_NF MBK_G_LOOP8X("", "", "", "", "")

// ---- same scheme with 16 steps per group (6.125 slots per step; one trip = 32 steps).  Used for the blocks that
// hardly ever trip the test (interior of the set).
#define MBK_G_T2T4 MBK_G_T2T MBK_G_T2T MBK_G_T2T MBK_G_T2T
#define MBK_G_GROUP16(FIRST, MID, LAST, AD, BD, ID)        \
    FIRST MBK_G_T2T4 MBK_G_T2T MBK_G_T2T MBK_G_T2T MID MBK_G_T2T4 MBK_G_T2T MBK_G_T2T MBK_G_T2T LAST \
    "v_add_" MBK_F " %[m], " AD ", " BD "\n"                     \
    "v_cmp_ngt_" MBK_F " vcc, 4.0, %[m]\n"                       \
    "s_cbranch_vccnz .Lgrep" ID "_%=\n"                    \
    ".Lgcont" ID "_%=:\n"
#define MBK_G_LOOP16X(INIT, MID1, CYC1, MID2, CYC2, OOL, FIX)                      \
    "s_mov_b64 %[save], exec\n"                            \
    "s_mov_b32 %[n], %[n0]\n"                              \
    INIT                                                   \
    "s_cmp_ge_u32 %[n], %[limit8]\n"                       \
    "s_cbranch_scc1 .Lgtail_%=\n"                          \
    ".Lgmain_%=:\n"                                        \
    MBK_G_GROUP16(MBK_G_A2T, MID1, MBK_G_T2B, "%[a2]", "%[b2]", "1") \
    CYC1                                                   \
    MBK_G_GROUP16(MBK_G_B2T, MID2, MBK_G_T2A, "%[a]", "%[b]", "2")   \
    CYC2                                                   \
    "s_add_u32 %[n], %[n], 32\n"                           \
    "s_cmp_lt_u32 %[n], %[limit8]\n"                       \
    "s_cbranch_scc1 .Lgmain_%=\n"                          \
    ".Lgtail_%=:\n"                                        \
    "s_cmp_ge_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgdone_%=\n"                          \
    ".Lgtloop_%=:\n"                                       \
    MBK_STEP_HEAD_FMA MBK_STEP_TAIL("GT")                  \
    "s_add_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lt_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgtloop_%=\n"                         \
    "s_branch .Lgdone_%=\n"                                \
    MBK_G_TRIP_A("1", "0")                                 \
    MBK_G_TRIP_B("2", "16")                                \
    MBK_ESCAPE("GT", "1")                                  \
    OOL                                                    \
    ".Ldone_%=:\n"                                         \
    ".Lgdone_%=:\n"                                        \
    "s_mov_b64 exec, %[save]\n"                            \
    FIX                                                    \
    "s_mov_b64 exec, %[save]\n"
#define MBK_G_LOOP16 MBK_G_LOOP16X("", "", "", "", "", "", MBK_G_FIXUP("16"))
#define MBK_G_LOOP16_NF MBK_G_LOOP16X("", "", "", "", "", "", "")

// ---- 32 steps per group (6.0625 slots per step; one trip = 64 steps): strict loops only (round 3).  Not offered with
// the cycle test: its checks every 8 steps would put THREE consecutive checks inside a group, between two bailout
// tests, and the argument that makes a mid-group match sound (one of the two states compared has been through a test
// since -- see "cycle detection" below) needs a test between any two checks; without it two untested NaN states of
// an escaped lane could compare equal.
#define MBK_G_T2T7 MBK_G_T2T4 MBK_G_T2T MBK_G_T2T MBK_G_T2T
#define MBK_G_GROUP32(FIRST, LAST, AD, BD, ID)             \
    FIRST MBK_G_T2T7 MBK_G_T2T4 MBK_G_T2T4 MBK_G_T2T4 MBK_G_T2T4 MBK_G_T2T7 LAST \
    "v_add_" MBK_F " %[m], " AD ", " BD "\n"                     \
    "v_cmp_ngt_" MBK_F " vcc, 4.0, %[m]\n"                       \
    "s_cbranch_vccnz .Lgrep" ID "_%=\n"                    \
    ".Lgcont" ID "_%=:\n"
#define MBK_G_LOOP32                                       \
    "s_mov_b64 %[save], exec\n"                            \
    "s_mov_b32 %[n], %[n0]\n"                              \
    "s_cmp_ge_u32 %[n], %[limit8]\n"                       \
    "s_cbranch_scc1 .Lgtail_%=\n"                          \
    ".Lgmain_%=:\n"                                        \
    MBK_G_GROUP32(MBK_G_A2T, MBK_G_T2B, "%[a2]", "%[b2]", "1") \
    MBK_G_GROUP32(MBK_G_B2T, MBK_G_T2A, "%[a]", "%[b]", "2")   \
    "s_add_u32 %[n], %[n], 64\n"                           \
    "s_cmp_lt_u32 %[n], %[limit8]\n"                       \
    "s_cbranch_scc1 .Lgmain_%=\n"                          \
    ".Lgtail_%=:\n"                                        \
    "s_cmp_ge_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgdone_%=\n"                          \
    ".Lgtloop_%=:\n"                                       \
    MBK_STEP_HEAD_FMA MBK_STEP_TAIL("GT")                  \
    "s_add_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lt_u32 %[n], %[total]\n"                        \
    "s_cbranch_scc1 .Lgtloop_%=\n"                         \
    "s_branch .Lgdone_%=\n"                                \
    MBK_G_TRIP_A("1", "0")                                 \
    MBK_G_TRIP_B("2", "32")                                \
    MBK_ESCAPE("GT", "1")                                  \
    ".Ldone_%=:\n"                                         \
    ".Lgdone_%=:\n"                                        \
    "s_mov_b64 exec, %[save]\n"                            \
    MBK_G_FIXUP("32")                                      \
    "s_mov_b64 exec, %[save]\n"

// ---- cycle detection (MBK_OPT_CYCLE_DETECT; the "C" variants of the 8- and 16-step loops) -----------------
// A pixel of the set costs the reference mrd-1 steps and ends as 0.  The step map z -> z^2 + c is a
// deterministic function of the (zr, zi) bit patterns, so a lane whose state is BITWISE equal to an earlier
// state of its own orbit is on a cycle it can never leave; no state of that cycle trips the bailout (every
// group end between the two visits passed the grouped test, and ">= 4 stays >= 4" covers the steps between
// group ends), so the reference's loop runs to mrd-1 for it and returns 0 -- and the lane may stop now.
// Orbits attracted to a cycle do become bitwise periodic in fp64 once the contraction has pushed the error
// below one ulp (|multiplier| 0.5: ~50 steps; 0.9: ~350).  Brent's scheme: every 8 steps (round 3; every 16 in
// round 2 -- a period p is caught lcm(8, p) steps after the orbit has settled instead of lcm(16, p)) compare the
// state with a saved one (2 integer compares per 8 steps: 6.125 -> 6.375 issue slots per step); the saved state is
// replaced after 1, 2, 4, 8, ... checks, so any period is caught once the window is long enough and the
// orbit has settled.  In the 16-step groups every other check sits in the MIDDLE of a group, on the scratch set:
// that state has not been through a bailout test yet, but it is compared with a saved state that has (a lane that
// is still alive passed a group-end test after the saved state was taken, and ">= 4 stays >= 4" runs backwards:
// a group end below 4 means every earlier state was below 4), so a bitwise match proves the current state valid too.  Retired lanes get cnt = -1 (mapped to 0 by escape_count_group) and leave EXEC; the
// wave leaves when EXEC is empty.  Nothing is approximate: a lane that is not exactly periodic just runs on.
// On BASELINE cfg2 this retires 79 % of the never-escaping pixels early and halves the wave-steps of the
// tile (47.3 M -> 23.6 M, CPU model in scripts/cycle_model.py); deep zooms gain little and pay the 2 %.
// WINDOW SCHEDULE (round 5, MBK_OPT_CYCLE_WINDOW).  A lane whose orbit becomes bitwise periodic at step s retires at the
// first reference state taken at or after s whose window spans lcm(8, period) steps, plus that lcm.  Doubled windows put the
// reference states at steps 8, 16, 32, 64, ...: on average 1.44 s.  Any schedule is exact (a bitwise repeat proves the
// cycle whatever the two steps are), and the bitwise periods of a full-set view are short (cfg2: 1, 2, 3, 4, 5 make up
// 87 % of the settled pixels, scripts/cycle_window_model.c), so the windows grow by a quarter (+ 1) while they are shorter than
// `wcap` checks -- reference states at checks 1, 3, 6, 10, 16, 24, 35, 49, 67, 90, 119 ... -- and double from there on, which
// keeps Brent's guarantee for the long periods of deep zooms: on the exact counts cfg2 and the level-1 / level-4 DataChunks
// lose 6.4-7.0 % of their wave-steps, cfg5 5.4 %, cfg3 (whose periods need the long windows) +0.2 %.  Growing by a quarter for
// ever would cost cfg3 9 %, growing by half 2 %.
#define MBK_G_CYC_INIT                                     \
    "v_mov_" MBK_CYC_MOV " %[szr], %[zr]\n"                \
    "v_mov_" MBK_CYC_MOV " %[szi], %[zi]\n"                \
    "s_mov_b32 %[tc], 0\n"                                 \
    "s_mov_b32 %[win], 1\n"
// (the second pass of SPILL resumes orbits that have n0 steps behind them: its window starts where the schedule would stand by
// then, not at 1 -- escape_steps_group's kWin0)
#define MBK_G_CYC_INIT_W                                   \
    "v_mov_" MBK_CYC_MOV " %[szr], %[zr]\n"                \
    "v_mov_" MBK_CYC_MOV " %[szi], %[zi]\n"                \
    "s_mov_b32 %[tc], 0\n"                                 \
    "s_mov_b32 %[win], %[win0]\n"
#define MBK_G_CYC(ZR, ZI, ID)                              \
    "v_cmp_eq_" MBK_CYC_BITS " vcc, " ZR ", %[szr]\n"      \
    "v_cmp_eq_" MBK_CYC_BITS "_e64 %[tmp2], " ZI ", %[szi]\n" \
    "s_and_b64 vcc, vcc, %[tmp2]\n"                        \
    "s_cbranch_vccnz .Lcyc" ID "_%=\n"                     \
    ".Lcyccont" ID "_%=:\n"                                \
    "s_add_u32 %[tc], %[tc], 1\n"                          \
    "s_cmp_ge_u32 %[tc], %[win]\n"                         \
    "s_cbranch_scc1 .Lcycsave" ID "_%=\n"                  \
    ".Lcycsaved" ID "_%=:\n"
// out of line: retire the lanes in VCC (cnt = -1); take a new reference state and lengthen the window:
// win += win < wcap ? win / 4 + 1 : win   (wcap = 0: always doubled, rounds 2-4; the WINDOW SCHEDULE comment above)
#define MBK_G_CYC_OOL(ZR, ZI, ID)                          \
    ".Lcyc" ID "_%=:\n"                                    \
    "s_and_saveexec_b64 %[tmp], vcc\n"                     \
    "v_mov_b32 %[cnt], -1\n"                               \
    "s_andn2_b64 exec, %[tmp], vcc\n"                      \
    "s_cbranch_scc1 .Lcyccont" ID "_%=\n"                  \
    "s_branch .Lgdone_%=\n"                                \
    ".Lcycsave" ID "_%=:\n"                                \
    "v_mov_" MBK_CYC_MOV " %[szr], " ZR "\n"               \
    "v_mov_" MBK_CYC_MOV " %[szi], " ZI "\n"               \
    "s_mov_b32 %[tc], 0\n"                                 \
    "s_lshr_b32 %[k], %[win], 2\n"                         \
    "s_add_u32 %[k], %[k], 1\n"                            \
    "s_cmp_lt_u32 %[win], %[wcap]\n"                       \
    "s_cselect_b32 %[k], %[k], %[win]\n"                   \
    "s_add_u32 %[win], %[win], %[k]\n"                     \
    "s_branch .Lcycsaved" ID "_%=\n"
#define MBK_G_LOOP8CXI(INIT, FIX) MBK_G_LOOP8X(INIT, MBK_G_CYC("%[zr2]", "%[zi2]", "1"), MBK_G_CYC("%[zr]", "%[zi]", "2"), \
                                               MBK_G_CYC_OOL("%[zr2]", "%[zi2]", "1") MBK_G_CYC_OOL("%[zr]", "%[zi]", "2"), FIX)
#define MBK_G_LOOP8CX(FIX) MBK_G_LOOP8CXI(MBK_G_CYC_INIT, FIX)
#define MBK_G_LOOP8C_W MBK_G_LOOP8CXI(MBK_G_CYC_INIT_W, MBK_G_FIXUP("8"))
#define MBK_G_LOOP16CX(FIX) MBK_G_LOOP16X(MBK_G_CYC_INIT, MBK_G_CYC("%[zrt]", "%[zit]", "M1"), MBK_G_CYC("%[zr2]", "%[zi2]", "1"), \
                                          MBK_G_CYC("%[zrt]", "%[zit]", "M2"), MBK_G_CYC("%[zr]", "%[zi]", "2"), \
                                          MBK_G_CYC_OOL("%[zrt]", "%[zit]", "M1") MBK_G_CYC_OOL("%[zr2]", "%[zi2]", "1") \
                                          MBK_G_CYC_OOL("%[zrt]", "%[zit]", "M2") MBK_G_CYC_OOL("%[zr]", "%[zi]", "2"), FIX)
#define MBK_G_LOOP8C MBK_G_LOOP8CX(MBK_G_FIXUP("8"))
#define MBK_G_LOOP16C MBK_G_LOOP16CX(MBK_G_FIXUP("16"))
#define MBK_G_LOOP8C_NF MBK_G_LOOP8CX("")
#define MBK_G_LOOP16C_NF MBK_G_LOOP16CX("")
// (carry form, escape_steps_carry: no INIT either -- the reference state, the check counter and the window come in and go out, so
// that a block whose steps run in several stretches keeps ONE schedule of the cycle test across them)
#define MBK_G_LOOP8C_R MBK_G_LOOP8CXI("", "")
#define MBK_G_LOOP16C_R MBK_G_LOOP16X("", MBK_G_CYC("%[zrt]", "%[zit]", "M1"), MBK_G_CYC("%[zr2]", "%[zi2]", "1"), \
                                      MBK_G_CYC("%[zrt]", "%[zit]", "M2"), MBK_G_CYC("%[zr]", "%[zi]", "2"), \
                                      MBK_G_CYC_OOL("%[zrt]", "%[zit]", "M1") MBK_G_CYC_OOL("%[zr2]", "%[zi2]", "1") \
                                      MBK_G_CYC_OOL("%[zrt]", "%[zit]", "M2") MBK_G_CYC_OOL("%[zr]", "%[zi]", "2"), "")

// Grouped loop on an existing state: steps n0+1 .. total (see escape_steps_asm for the contract).
// kCycle: the variant with cycle detection (8- and 16-step groups only); lanes it retires carry cnt = -1.
// kFixup = false (8- and 16-step groups): without the deferred replay at the end -- the caller runs escape_fixup itself, once.
// kWin0 (8-step groups with the cycle test and the fix-up): the window of the first reference state is cyc_win0 checks, not 1.
template <int kGroup = 4, bool kCycle = false, bool kFixup = true, bool kWin0 = false>
__device__ __forceinline__ void escape_steps_group(MBK_T cr, MBK_T ci, MBK_T &zr, MBK_T &zi, MBK_T &a,
                                                   MBK_T &b, MBK_T &m, int32_t &cnt, uint32_t n0, uint32_t total,
                                                   uint32_t cyc_wcap = 32u, uint32_t cyc_win0 = 1u)
{
    static_assert(kFixup || kGroup == 8 || kGroup == 16, "the form without the fix-up exists for 8- and 16-step groups");
    static_assert(!kWin0 || (kGroup == 8 && kCycle && kFixup), "a starting window exists for the 8-step cycle-test loop");
    // m: as in escape_steps_asm -- a lane that escapes does so in a replay step (or the tail loop) and
    // is masked off right after, so its m is the |z|^2 of its first escaping step
    MBK_T zr2, zi2, a2, b2, zrt, zit, at, bt, t, p;
    const uint32_t limit8 = n0 + ((total - n0) & (kGroup == 32 ? ~63u : kGroup == 16 ? ~31u : kGroup == 8 ? ~15u : ~7u));  // whole trips only
    uint32_t n, k;
    unsigned long long save, tmp, tmp2;
#define MBK_G_OUTPUTS                                                                           \
                   [zr] "+&v"(zr), [zi] "+&v"(zi), [a] "+&v"(a), [b] "+&v"(b), [cnt] "+&v"(cnt),  \
                   [zr2] "=&v"(zr2), [zi2] "=&v"(zi2), [a2] "=&v"(a2), [b2] "=&v"(b2),            \
                   [zrt] "=&v"(zrt), [zit] "=&v"(zit), [at] "=&v"(at), [bt] "=&v"(bt),            \
                   [m] "+&v"(m), [t] "=&v"(t), [p] "=&v"(p), [n] "=&s"(n), [k] "=&s"(k),           \
                   [save] "=&s"(save), [tmp] "=&s"(tmp), [tmp2] "=&s"(tmp2)
#define MBK_G_INPUTS [cr] "v"(cr), [ci] "v"(ci), [total] "s"(total), [limit8] "s"(limit8), [n0] "s"(n0)
    if (kCycle && kGroup >= 8) {
        MBK_T szr, szi;    // the reference state of the cycle test
        uint32_t tc, win;  // checks since it was taken / checks until it is replaced
        if (kGroup == 16 && kFixup) {
            asm volatile(MBK_G_LOOP16C
                         : MBK_G_OUTPUTS, [szr] "=&v"(szr), [szi] "=&v"(szi), [tc] "=&s"(tc), [win] "=&s"(win)
                         : MBK_G_INPUTS, [wcap] "s"(cyc_wcap)
                         : "vcc", "scc");
        } else if (kGroup == 16) {
            asm volatile(MBK_G_LOOP16C_NF
                         : MBK_G_OUTPUTS, [szr] "=&v"(szr), [szi] "=&v"(szi), [tc] "=&s"(tc), [win] "=&s"(win)
                         : MBK_G_INPUTS, [wcap] "s"(cyc_wcap)
                         : "vcc", "scc");
        } else if (kWin0) {
            asm volatile(MBK_G_LOOP8C_W
                         : MBK_G_OUTPUTS, [szr] "=&v"(szr), [szi] "=&v"(szi), [tc] "=&s"(tc), [win] "=&s"(win)
                         : MBK_G_INPUTS, [wcap] "s"(cyc_wcap), [win0] "s"(cyc_win0)
                         : "vcc", "scc");
        } else if (kFixup) {
            asm volatile(MBK_G_LOOP8C
                         : MBK_G_OUTPUTS, [szr] "=&v"(szr), [szi] "=&v"(szi), [tc] "=&s"(tc), [win] "=&s"(win)
                         : MBK_G_INPUTS, [wcap] "s"(cyc_wcap)
                         : "vcc", "scc");
        } else {
            asm volatile(MBK_G_LOOP8C_NF
                         : MBK_G_OUTPUTS, [szr] "=&v"(szr), [szi] "=&v"(szi), [tc] "=&s"(tc), [win] "=&s"(win)
                         : MBK_G_INPUTS, [wcap] "s"(cyc_wcap)
                         : "vcc", "scc");
        }
    } else if (kGroup == 32) {
        asm volatile(MBK_G_LOOP32 : MBK_G_OUTPUTS : MBK_G_INPUTS : "vcc", "scc");
    } else if (kGroup == 16 && kFixup) {
        asm volatile(MBK_G_LOOP16 : MBK_G_OUTPUTS : MBK_G_INPUTS : "vcc", "scc");
    } else if (kGroup == 16) {
        asm volatile(MBK_G_LOOP16_NF : MBK_G_OUTPUTS : MBK_G_INPUTS : "vcc", "scc");
    } else if (kGroup == 8 && kFixup) {
        asm volatile(MBK_G_LOOP8 : MBK_G_OUTPUTS : MBK_G_INPUTS : "vcc", "scc");
    } else if (kGroup == 8) {
        asm volatile(MBK_G_LOOP8_NF : MBK_G_OUTPUTS : MBK_G_INPUTS : "vcc", "scc");
    } else {
        asm volatile(MBK_G_LOOP : MBK_G_OUTPUTS : MBK_G_INPUTS : "vcc", "scc");
    }
#undef MBK_G_OUTPUTS
#undef MBK_G_INPUTS
}

// Steps n0+1 .. total with the cycle test CARRIED: (szr, szi) the reference state, tc the checks since it was taken, win the
// checks until it is replaced come in (the caller starts with szr = zr, szi = zi, tc = 0, win = 1: what MBK_G_CYC_INIT does) and go
// out, and there is no fix-up at the end (kFixup = false above).  For block_pixel_spill: its stretches between checkpoints
// restarted the window at 1 each time, which cost the cycle-test leg of cfg3 what finer checkpoints made visible (+6 %).
// A bitwise match with a reference state taken in an earlier stretch proves the cycle like any other.  Whole 32-step trips in
// 16-step groups (kGroup 16), then whole 16-step trips in 8-step groups, then single steps.
template <int kGroup>
__device__ __forceinline__ void escape_steps_carry(MBK_T cr, MBK_T ci, MBK_T &zr, MBK_T &zi, MBK_T &a, MBK_T &b, MBK_T &m, int32_t &cnt,
                                                   uint32_t n0, uint32_t total, uint32_t cyc_wcap, MBK_T &szr, MBK_T &szi, uint32_t &tc, uint32_t &win)
{
    static_assert(kGroup == 8 || kGroup == 16, "8- or 16-step groups");
    MBK_T zr2, zi2, a2, b2, zrt, zit, at, bt, t, p;
    uint32_t n, k;
    unsigned long long save, tmp, tmp2;
#define MBK_G_CARRY_OPERANDS                                                                       \
                 : [zr] "+&v"(zr), [zi] "+&v"(zi), [a] "+&v"(a), [b] "+&v"(b), [cnt] "+&v"(cnt),    \
                   [zr2] "=&v"(zr2), [zi2] "=&v"(zi2), [a2] "=&v"(a2), [b2] "=&v"(b2),              \
                   [zrt] "=&v"(zrt), [zit] "=&v"(zit), [at] "=&v"(at), [bt] "=&v"(bt),              \
                   [m] "+&v"(m), [t] "=&v"(t), [p] "=&v"(p), [n] "=&s"(n), [k] "=&s"(k),             \
                   [save] "=&s"(save), [tmp] "=&s"(tmp), [tmp2] "=&s"(tmp2),                        \
                   [szr] "+&v"(szr), [szi] "+&v"(szi), [tc] "+&s"(tc), [win] "+&s"(win)              \
                 : [cr] "v"(cr), [ci] "v"(ci), [total] "s"(stop), [limit8] "s"(limit8), [n0] "s"(start), [wcap] "s"(cyc_wcap) \
                 : "vcc", "scc"
    uint32_t start = n0;
    if (kGroup == 16) {
        const uint32_t stop = n0 + ((total - n0) & ~31u), limit8 = stop;     // whole 32-step trips only: no single steps here
        if (stop > start) {
            asm volatile(MBK_G_LOOP16C_R MBK_G_CARRY_OPERANDS);
            tc = (uint32_t)__builtin_amdgcn_readfirstlane((int)tc);
            win = (uint32_t)__builtin_amdgcn_readfirstlane((int)win);
        }
        start = stop;
    }
    if (total > start) {
        const uint32_t stop = total, limit8 = start + ((total - start) & ~15u);
        if (cnt == 0) {
            asm volatile(MBK_G_LOOP8C_R MBK_G_CARRY_OPERANDS);
        }
        tc = (uint32_t)__builtin_amdgcn_readfirstlane((int)tc);
        win = (uint32_t)__builtin_amdgcn_readfirstlane((int)win);
    }
#undef MBK_G_CARRY_OPERANDS
}

// The deferred replay on its own: every lane that is pending (cnt < 0 with bit 31 as the mark, not -1 = retired by the cycle
// test) runs up to 16 exact steps from the group-start state it holds in (zr, zi, a, b) and takes the step of its first hit --
// MBK_G_FIXUP, what the loops above end with, for callers that ran them in the form without it.  16 covers both group sizes:
// a lane that tripped an 8-step group finds its hit within 8.
__device__ __forceinline__ void escape_fixup(MBK_T cr, MBK_T ci, MBK_T &zr, MBK_T &zi, MBK_T &a, MBK_T &b, MBK_T &m, int32_t &cnt)
{
    MBK_T t, p;
    uint32_t k;
    unsigned long long save, tmp2;
    asm volatile("s_mov_b64 %[save], exec\n"
                 MBK_G_FIXUP("16")
                 "s_mov_b64 exec, %[save]\n"
                 : [zr] "+&v"(zr), [zi] "+&v"(zi), [a] "+&v"(a), [b] "+&v"(b), [cnt] "+&v"(cnt), [m] "+&v"(m), [t] "=&v"(t), [p] "=&v"(p),
                   [k] "=&s"(k), [save] "=&s"(save), [tmp2] "=&s"(tmp2)
                 : [cr] "v"(cr), [ci] "v"(ci)
                 : "vcc", "scc");
}

// Steps n0+1 .. total with kGroup-step groups; for 16-step groups the remainder (up to 31 steps) is not left to
// the per-step tail (8 slots per step) but run in 8-step groups first: whole 32-step trips, then whole
// 16-step trips of 8-step groups, then fewer than 16 single steps.
template <int kGroup, bool kCycle = false, bool kFixup = true>
__device__ __forceinline__ void escape_steps_tail(MBK_T cr, MBK_T ci, MBK_T &zr, MBK_T &zi, MBK_T &a, MBK_T &b,
                                                  MBK_T &m, int32_t &cnt, uint32_t n0, uint32_t total, uint32_t cyc_wcap = 32u)
{
    if (kGroup == 32) {   // whole 64-step trips, then the rest (< 64 steps) as the 16-step form runs it
        static_assert(kGroup != 32 || !kCycle, "32-step groups have no cycle test");
        const uint32_t t64 = n0 + ((total - n0) & ~63u);
        if (t64 > n0) escape_steps_group<32, false>(cr, ci, zr, zi, a, b, m, cnt, n0, t64);
        if (cnt == 0 && total > t64) escape_steps_tail<16, false>(cr, ci, zr, zi, a, b, m, cnt, t64, total);
    } else if (kGroup == 16) {
        const uint32_t t32 = n0 + ((total - n0) & ~31u);
        if (t32 > n0) escape_steps_group<16, kCycle, kFixup>(cr, ci, zr, zi, a, b, m, cnt, n0, t32, cyc_wcap);
        if (cnt == 0 && total > t32) escape_steps_group<8, kCycle, kFixup>(cr, ci, zr, zi, a, b, m, cnt, t32, total, cyc_wcap);
    } else {
        escape_steps_group<kGroup, kCycle, kFixup>(cr, ci, zr, zi, a, b, m, cnt, n0, total, cyc_wcap);
    }
}

// Default pixel routine: the first kExactSteps steps with the per-step test (most escaping pixels leave
// here and never pay a group + replay), the rest in groups.
template <int kGroup = 4, bool kCycle = false>
__device__ __forceinline__ int32_t escape_count_group(MBK_T cr, MBK_T ci, int32_t mrd, MBK_T *m_out = nullptr,
                                                      uint32_t kExactSteps = 8, uint32_t cyc_wcap = 32u)
{
    MBK_T zr = cr, zi = ci;
    MBK_T a = zr * zr, b = zi * zi, m = 0;
    int32_t cnt = 0;
    const uint32_t total = mrd > 1 ? (uint32_t)mrd - 1u : 0u;
    const uint32_t first = total < kExactSteps ? total : kExactSteps;
    escape_steps_asm<true>(cr, ci, zr, zi, a, b, m, cnt, 0u, first);
    if (cnt == 0 && total > first) escape_steps_tail<kGroup, kCycle>(cr, ci, zr, zi, a, b, m, cnt, first, total, cyc_wcap);
    if (m_out) *m_out = m;
    return kCycle && cnt < 0 ? 0 : cnt;   // -1: retired by the cycle test = never escapes
}

// ---- the test-free loop (MBK_OPT_SURE_INTERIOR; block_pixel's certified blocks) ---------------------------------
// Steps 1 .. total from z = c, every one the in-place step MBK_G_A2A: 6 arithmetic instructions and nothing else -- no m, no
// compare, no trip label, no cnt -- in trips of 32 on a scalar counter, the remainder (total mod 32) as single steps, untested
// too.  ONE NaN-inclusive test behind the last step stands for all the tests the grouped loop would have made on the way:
// "once |z|^2 >= 4 it stays >= 4 and ends in inf, then NaN" (the grouped test's invariant above; it needs |c| <= 2 - 1e-9, which
// the caller guarantees), so a lane that would have tripped any of them trips this one.  Returns the wave's trip mask.  Zero:
// no lane of the wave ever escaped, every count is 0.  Non-zero: the state is worthless (nobody knows WHEN a lane left) and the
// caller runs the block again with the grouped loop.  Operand order as in the grouped steps, so every (zr, zi) on the way is
// the one the grouped loop computes.  total >= 1: z = c itself is never tested.
#define MBK_G_A2A4 MBK_G_A2A MBK_G_A2A MBK_G_A2A MBK_G_A2A
#define MBK_G_A2A32 MBK_G_A2A4 MBK_G_A2A4 MBK_G_A2A4 MBK_G_A2A4 MBK_G_A2A4 MBK_G_A2A4 MBK_G_A2A4 MBK_G_A2A4
#define MBK_SURE_LOOP                                      \
    "s_lshr_b32 %[n], %[total], 5\n"                       \
    "s_cmp_eq_u32 %[n], 0\n"                               \
    "s_cbranch_scc1 .Lsrem_%=\n"                           \
    ".Lsmain_%=:\n"                                        \
    MBK_G_A2A32                                            \
    "s_sub_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lg_u32 %[n], 0\n"                               \
    "s_cbranch_scc1 .Lsmain_%=\n"                          \
    ".Lsrem_%=:\n"                                         \
    "s_and_b32 %[n], %[total], 31\n"                       \
    "s_cmp_eq_u32 %[n], 0\n"                               \
    "s_cbranch_scc1 .Lsend_%=\n"                           \
    ".Lsone_%=:\n"                                         \
    MBK_G_A2A                                              \
    "s_sub_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lg_u32 %[n], 0\n"                               \
    "s_cbranch_scc1 .Lsone_%=\n"                           \
    ".Lsend_%=:\n"                                         \
    "v_add_" MBK_F " %[m], %[a], %[b]\n"                   \
    "v_cmp_ngt_" MBK_F " vcc, 4.0, %[m]\n"                 \
    "s_mov_b64 %[mask], vcc\n"
__device__ __forceinline__ unsigned long long escape_steps_sure(MBK_T cr, MBK_T ci, uint32_t total)
{
    MBK_T zr = cr, zi = ci;
    MBK_T a = zr * zr, b = zi * zi, m, t, p;
    uint32_t n;
    unsigned long long mask;
    asm volatile(MBK_SURE_LOOP
                 : [zr] "+&v"(zr), [zi] "+&v"(zi), [a] "+&v"(a), [b] "+&v"(b), [m] "=&v"(m), [t] "=&v"(t), [p] "=&v"(p),
                   [n] "=&s"(n), [mask] "=&s"(mask)
                 : [cr] "v"(cr), [ci] "v"(ci), [total] "s"(total)
                 : "vcc", "scc");
    return mask;
}

// The same two routines for an orbit that starts at z0 = (z0r, z0i) instead of c: the Julia set of the parameter c (mbk_julia.h).
// The step loops above keep state and parameter apart; only the seed differs.  z0 is never tested, as c is not above.  What the
// grouped test and the cycle test rest on carries over: ">= 4 stays >= 4" needs |c| <= 2 - 1e-9 and nothing of z (the caller
// sends every other c to the per-step loop), and the step map is a function of the state alone once c is fixed.
template <bool kFmaDouble>
__device__ __forceinline__ int32_t escape_count_asm_from(MBK_T z0r, MBK_T z0i, MBK_T cr, MBK_T ci, int32_t mrd, MBK_T *m_out = nullptr)
{
    MBK_T zr = z0r, zi = z0i;
    MBK_T a = zr * zr, b = zi * zi, m = 0;
    int32_t cnt = 0;
    escape_steps_asm<kFmaDouble>(cr, ci, zr, zi, a, b, m, cnt, 0u, mrd > 1 ? (uint32_t)mrd - 1u : 0u);
    if (m_out) *m_out = m;
    return cnt;
}

template <int kGroup = 8, bool kCycle = false>
__device__ __forceinline__ int32_t escape_count_group_from(MBK_T z0r, MBK_T z0i, MBK_T cr, MBK_T ci, int32_t mrd, MBK_T *m_out = nullptr,
                                                           uint32_t kExactSteps = 8, uint32_t cyc_wcap = 32u)
{
    MBK_T zr = z0r, zi = z0i;
    MBK_T a = zr * zr, b = zi * zi, m = 0;
    int32_t cnt = 0;
    const uint32_t total = mrd > 1 ? (uint32_t)mrd - 1u : 0u;
    const uint32_t first = total < kExactSteps ? total : kExactSteps;
    escape_steps_asm<true>(cr, ci, zr, zi, a, b, m, cnt, 0u, first);
    if (cnt == 0 && total > first) escape_steps_tail<kGroup, kCycle>(cr, ci, zr, zi, a, b, m, cnt, first, total, cyc_wcap);
    if (m_out) *m_out = m;
    return kCycle && cnt < 0 ? 0 : cnt;   // -1: retired by the cycle test = never escapes
}

// ---------------------------------------------------------------------------------------------
// The light path of pass 1 (kernel "scan") for a RUN of interior 8x8 blocks, in one asm loop: block k of the run lies
// `rowinc` rows below block k-1 in the same block column (the wave's stride), so per block only the imaginary
// coordinate changes (np.linspace arithmetic: fl(fl(row*step)+start); the caller guarantees that no block of the run
// holds the axis' pinned end point).  Per block: coordinate, up to four steps of the reference loop with the
// reference's own test (WorkerCUDA.py:47-66: a lane whose |z|^2 >= 4 takes its step index and LEAVES -- EXEC is
// narrowed to the lanes still inside, so nothing here relies on ">= 4 stays >= 4" and no |c| = 2 ring check is
// needed: round 2's branch-free form spent 3 of its ~30 VALU instructions per block on that check), and -- when no
// lane is left inside -- the stores, addressed as uniform base + 32-bit lane offset; then row and offset advance
// and the loop goes on.  ~22 VALU and ~12 scalar instructions for a block whose pixels are gone after two steps.  Why
// one loop: the CU's scalar unit issues one instruction per cycle for all four SIMDs, as many as the four vector ALUs
// together; with the compiler's loop around a per-block asm body a block cost ~33 scalar instructions for ~30 VALU
// and the pass was scalar-bound (product 19.8 us for the all-exterior tile against 15.3 us for the bare body in
// profiles/microbench/light_path.hip).
// The quantised byte of a count in 1..4 comes from a packed table (qtab, byte k-1 = quantise(k)).
// On return: 0 = all n blocks finished and stored (n = 0).  1 = the block that row / off now point at has lanes still
// inside after 4 steps; nothing was stored for it, cnt = 5 marks those lanes (others: their escape step), n counts
// the blocks left including this one.  `off` is the lane's offset from the base pointers, in bytes of the int32
// output when kCounts (the byte output then uses off >> 2), in elements otherwise; `einc` is its increment per block.
// ---------------------------------------------------------------------------------------------
#define MBK_LR_TEST                                        \
    "v_mul_" MBK_F " %[a], %[zr], %[zr]\n"                 \
    "v_mul_" MBK_F " %[b], %[zi], %[zi]\n"                 \
    "v_add_" MBK_F " %[m], %[a], %[b]\n"                   \
    "v_cmp_gt_" MBK_F " vcc, 4.0, %[m]\n"                  \
    "v_addc_co_u32_e64 %[cnt], %[tmp], %[cnt], 0, vcc\n"   \
    "s_mov_b64 exec, vcc\n"                                \
    "s_cbranch_execz .Llrdone_%=\n"
#define MBK_LR_BODY(STORES)                                \
    "s_mov_b64 %[save], exec\n"                            \
    ".Llrblk_%=:\n"                                        \
    "v_cvt_f64_u32 %[t64], %[row]\n"                       \
    "v_mul_f64 %[t64], %[t64], %[step]\n"                  \
    MBK_CI_FROM_T64                                        \
    "v_mov_b32 %[cnt], 1\n"                                \
    "v_mul_" MBK_F " %[b], %[ci], %[ci]\n"                 \
    "v_add_" MBK_F " %[t], %[a0], -%[b]\n"                 \
    "v_mul_" MBK_F " %[p], %[cr], %[ci]\n"                 \
    "v_add_" MBK_F " %[zr], %[t], %[cr]\n"                 \
    "v_fma_" MBK_F " %[zi], %[p], 2.0, %[ci]\n"            \
    MBK_LR_TEST                                            \
    MBK_STEP_HEAD_FMA MBK_LR_TEST                          \
    MBK_STEP_HEAD_FMA MBK_LR_TEST                          \
    MBK_STEP_HEAD_FMA MBK_LR_TEST                          \
    "s_mov_b64 exec, %[save]\n"                            \
    "s_mov_b32 %[flag], 1\n"                               \
    "s_branch .Llrend_%=\n"                                \
    ".Llrdone_%=:\n"                                       \
    "s_mov_b64 exec, %[save]\n"                            \
    STORES                                                 \
    "v_add_u32 %[row], %[rowinc], %[row]\n"                \
    "v_add_u32 %[off], %[einc], %[off]\n"                  \
    "s_sub_u32 %[n], %[n], 1\n"                            \
    "s_cmp_lg_u32 %[n], 0\n"                               \
    "s_cbranch_scc1 .Llrblk_%=\n"                          \
    "s_mov_b32 %[flag], 0\n"                               \
    ".Llrend_%=:\n"
#define MBK_LR_ST_COUNTS "global_store_dword %[off], %[cnt], %[cbase]\n"
#define MBK_LR_ST_BYTES_Q                                  \
    "v_lshl_add_u32 %[q], %[cnt], 3, -8\n"                 \
    "v_lshrrev_b32_e64 %[q], %[q], %[qtab]\n"
#define MBK_LR_ST_BYTES_ONLY MBK_LR_ST_BYTES_Q "global_store_byte %[off], %[q], %[bbase]\n"
#define MBK_LR_ST_BOTH MBK_LR_ST_COUNTS MBK_LR_ST_BYTES_Q "v_lshrrev_b32 %[o2], 2, %[off]\nglobal_store_byte %[o2], %[q], %[bbase]\n"
// kAcc: `acc` (per lane) collects the counts of the blocks the run finished (the fused statistics of the
// finish-in-place form: 1 VALU instruction per block instead of a second pass over int32 counts in HBM).
template <bool kCounts, bool kBytes, bool kAcc = false>
__device__ __forceinline__ uint32_t escape_light_run(MBK_T cr, MBK_T a0, uint32_t &row, uint32_t rowinc, double im_step,
                                                     double im_start, int32_t &cnt, int32_t *cbase, uint8_t *bbase,
                                                     uint32_t &off, uint32_t einc, uint32_t qtab, uint32_t &n,
                                                     uint32_t *acc_io = nullptr)
{
    MBK_T ci, zr, zi, a, b, t, p, m;
    double t64;
    uint32_t q, o2, flag;
    unsigned long long tmp, save;
    const unsigned long long step_bits = (unsigned long long)__double_as_longlong(im_step);
    const unsigned long long start_bits = (unsigned long long)__double_as_longlong(im_start);
    uint32_t acc = kAcc ? *acc_io : 0u;
#define MBK_LR_OPERANDS                                                                                    \
        : [row] "+v"(row), [off] "+v"(off), [cnt] "=&v"(cnt), [n] "+s"(n), [acc] "+v"(acc), [ci] "=&v"(ci), [zr] "=&v"(zr), \
          [zi] "=&v"(zi), [a] "=&v"(a), [b] "=&v"(b), [m] "=&v"(m), [t] "=&v"(t), [p] "=&v"(p),            \
          [t64] "=&v"(t64), [q] "=&v"(q), [o2] "=&v"(o2), [tmp] "=&s"(tmp), [save] "=&s"(save),            \
          [flag] "=&s"(flag)                                                                               \
        : [cr] "v"(cr), [a0] "v"(a0), [step] "s"(step_bits), [start] "s"(start_bits), [cbase] "s"(cbase),  \
          [bbase] "s"(bbase), [qtab] "s"(qtab), [rowinc] "s"(rowinc), [einc] "s"(einc)                     \
        : "vcc", "scc", "memory"
#define MBK_LR_ACC "v_add_u32 %[acc], %[acc], %[cnt]\n"
    if (kAcc) {
        if (kCounts && kBytes) {
            asm volatile(MBK_LR_BODY(MBK_LR_ACC MBK_LR_ST_BOTH) MBK_LR_OPERANDS);
        } else if (kCounts) {
            asm volatile(MBK_LR_BODY(MBK_LR_ACC MBK_LR_ST_COUNTS) MBK_LR_OPERANDS);
        } else {
            asm volatile(MBK_LR_BODY(MBK_LR_ACC MBK_LR_ST_BYTES_ONLY) MBK_LR_OPERANDS);
        }
        *acc_io = acc;
    } else if (kCounts && kBytes) {
        asm volatile(MBK_LR_BODY(MBK_LR_ST_BOTH) MBK_LR_OPERANDS);
    } else if (kCounts) {
        asm volatile(MBK_LR_BODY(MBK_LR_ST_COUNTS) MBK_LR_OPERANDS);
    } else {
        asm volatile(MBK_LR_BODY(MBK_LR_ST_BYTES_ONLY) MBK_LR_OPERANDS);
    }
#undef MBK_LR_ACC
#undef MBK_LR_OPERANDS
    // (the compiler treats an asm result as divergent even when it lives in an SGPR; saying that they are
    // wave-uniform keeps the caller's loop -- counters, branches, base pointers -- on the scalar unit)
    n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)flag);
}
// ---------------------------------------------------------------------------------------------
// The light path for a ROW UNIT (round 4, kernel "units"): up to eight 8x8 blocks side by side in one block row -- the
// blocks whose bit is set in `mask` -- handled by one wave, one after the other.  Same arithmetic and the same exact
// EXEC-narrowing test as escape_light_run, with the roles of the axes swapped: the imaginary coordinate (and its square
// b0) is fixed for the unit, the real one is np.linspace's fl(fl(col*step)+start) per block (the caller guarantees
// that no block of the unit holds the axis' pinned end point or a ragged edge).  Why units: one single-wave workgroup
// per block costs 0.28 ns of the chip's one dispatcher and ~60 vector instructions of start-up per block, and
// cfg2 has 167 000 blocks that are gone after 3 steps -- a 50 us dispatch-bound phase at the end of every launch
// (profiles/r04/NOTES.md, scripts/fifo_model.py); eight such blocks per workgroup cost ~19 instructions each and an
// eighth of the dispatches.
// On return: 0 = every selected block from k on is finished and stored (k = 8).  1 = block k has lanes still inside
// after 4 steps: nothing was stored for it, the caller finishes it (block_pixel) and calls again with k + 1.
// `col` = this lane's column in the view for block k = 0 of the unit (the routine derives block k's from it), `off` =
// its store offset for block 0 (bytes of the int32 output when kCounts, elements otherwise), einc = the offset's
// increment per block (8 pixels).
// ---------------------------------------------------------------------------------------------
#define MBK_LW_TEST                                        \
    "v_mul_" MBK_F " %[a], %[zr], %[zr]\n"                 \
    "v_mul_" MBK_F " %[b], %[zi], %[zi]\n"                 \
    "v_add_" MBK_F " %[m], %[a], %[b]\n"                   \
    "v_cmp_gt_" MBK_F " vcc, 4.0, %[m]\n"                  \
    "v_addc_co_u32_e64 %[cnt], %[tmp], %[cnt], 0, vcc\n"   \
    "s_mov_b64 exec, vcc\n"                                \
    "s_cbranch_execz .Llwdone_%=\n"
#define MBK_LW_BODY(STORES)                                \
    "s_mov_b64 %[save], exec\n"                            \
    ".Llwblk_%=:\n"                                        \
    "s_bitcmp1_b32 %[mask], %[k]\n"                        \
    "s_cbranch_scc0 .Llwnext_%=\n"                         \
    "s_lshl_b32 %[kk], %[k], 3\n"                          \
    "v_add_u32 %[c], %[kk], %[col]\n"                      \
    "v_cvt_f64_u32 %[t64], %[c]\n"                         \
    "v_mul_f64 %[t64], %[t64], %[step]\n"                  \
    MBK_CR_FROM_T64                                        \
    "v_mov_b32 %[cnt], 1\n"                                \
    "v_mul_" MBK_F " %[a], %[cr], %[cr]\n"                 \
    "v_add_" MBK_F " %[t], %[a], -%[b0]\n"                 \
    "v_mul_" MBK_F " %[p], %[cr], %[ci]\n"                 \
    "v_add_" MBK_F " %[zr], %[t], %[cr]\n"                 \
    "v_fma_" MBK_F " %[zi], %[p], 2.0, %[ci]\n"            \
    MBK_LW_TEST                                            \
    MBK_STEP_HEAD_FMA MBK_LW_TEST                          \
    MBK_STEP_HEAD_FMA MBK_LW_TEST                          \
    MBK_STEP_HEAD_FMA MBK_LW_TEST                          \
    "s_mov_b64 exec, %[save]\n"                            \
    "s_mov_b32 %[flag], 1\n"                               \
    "s_branch .Llwend_%=\n"                                \
    ".Llwdone_%=:\n"                                       \
    "s_mov_b64 exec, %[save]\n"                            \
    "s_mul_i32 %[kk], %[k], %[einc]\n"                     \
    "v_add_u32 %[o], %[kk], %[off]\n"                      \
    STORES                                                 \
    ".Llwnext_%=:\n"                                       \
    "s_add_u32 %[k], %[k], 1\n"                            \
    "s_cmp_lt_u32 %[k], 8\n"                               \
    "s_cbranch_scc1 .Llwblk_%=\n"                          \
    "s_mov_b32 %[flag], 0\n"                               \
    ".Llwend_%=:\n"
#define MBK_LW_ST_COUNTS "global_store_dword %[o], %[cnt], %[cbase]\n"
#define MBK_LW_ST_BYTES_ONLY MBK_LR_ST_BYTES_Q "global_store_byte %[o], %[q], %[bbase]\n"
#define MBK_LW_ST_BOTH MBK_LW_ST_COUNTS MBK_LR_ST_BYTES_Q "v_lshrrev_b32 %[o2], 2, %[o]\nglobal_store_byte %[o2], %[q], %[bbase]\n"
// kAcc: `acc` (per lane) collects the counts of the blocks the unit finished (the fused statistics of a DataChunk launch).
template <bool kCounts, bool kBytes, bool kAcc = false>
__device__ __forceinline__ uint32_t escape_light_row(MBK_T ci, MBK_T b0, uint32_t col, double re_step, double re_start, int32_t &cnt,
                                                     int32_t *cbase, uint8_t *bbase, uint32_t off, uint32_t einc, uint32_t qtab,
                                                     uint32_t mask, uint32_t &k, uint32_t *acc_io = nullptr)
{
    MBK_T cr, zr, zi, a, b, t, p, m;
    double t64;
    uint32_t q, o, o2, c, flag, kk;
    unsigned long long tmp, save;
    const unsigned long long step_bits = (unsigned long long)__double_as_longlong(re_step);
    const unsigned long long start_bits = (unsigned long long)__double_as_longlong(re_start);
#define MBK_LW_OPERANDS                                                                                    \
        : [k] "+s"(k), [acc] "+v"(acc), [cnt] "=&v"(cnt), [cr] "=&v"(cr), [zr] "=&v"(zr), [zi] "=&v"(zi), [a] "=&v"(a), [b] "=&v"(b), \
          [m] "=&v"(m), [t] "=&v"(t), [p] "=&v"(p), [t64] "=&v"(t64), [q] "=&v"(q), [o] "=&v"(o), [o2] "=&v"(o2), \
          [c] "=&v"(c), [tmp] "=&s"(tmp), [save] "=&s"(save), [flag] "=&s"(flag), [kk] "=&s"(kk)             \
        : [ci] "v"(ci), [b0] "v"(b0), [col] "v"(col), [off] "v"(off), [step] "s"(step_bits), [start] "s"(start_bits), \
          [cbase] "s"(cbase), [bbase] "s"(bbase), [qtab] "s"(qtab), [einc] "s"(einc), [mask] "s"(mask)       \
        : "vcc", "scc", "memory"
    uint32_t acc = kAcc ? *acc_io : 0u;
    if (kAcc) {   // (the fused statistics exist for the bytes-only instantiation: a DataChunk whose caller wants no counts)
        asm volatile(MBK_LW_BODY("v_add_u32 %[acc], %[acc], %[cnt]\n" MBK_LW_ST_BYTES_ONLY) MBK_LW_OPERANDS);
        *acc_io = acc;
    } else if (kCounts && kBytes) {
        asm volatile(MBK_LW_BODY(MBK_LW_ST_BOTH) MBK_LW_OPERANDS);
    } else if (kCounts) {
        asm volatile(MBK_LW_BODY(MBK_LW_ST_COUNTS) MBK_LW_OPERANDS);
    } else {
        asm volatile(MBK_LW_BODY(MBK_LW_ST_BYTES_ONLY) MBK_LW_OPERANDS);
    }
#undef MBK_LW_OPERANDS
    k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)flag);
}
#undef MBK_LW_TEST
#undef MBK_LW_BODY
#undef MBK_LW_ST_COUNTS
#undef MBK_LW_ST_BYTES_ONLY
#undef MBK_LW_ST_BOTH

#undef MBK_LR_TEST
#undef MBK_LR_BODY
#undef MBK_LR_ST_COUNTS
#undef MBK_LR_ST_BYTES_Q
#undef MBK_LR_ST_BYTES_ONLY
#undef MBK_LR_ST_BOTH

#undef MBK_STEP_HEAD_FMA
#undef MBK_STEP_HEAD_SAFE
#undef MBK_STEP_TAIL
#undef MBK_ESCAPE
#undef MBK_LOOP_ASM
#undef MBK_G_STEP
#undef MBK_G_A2T
#undef MBK_G_B2T
#undef MBK_G_T2T
#undef MBK_G_T2A
#undef MBK_G_T2B
#undef MBK_G_GROUP
#undef MBK_G_TRIP_A
#undef MBK_G_TRIP_B
#undef MBK_G_A2A
#undef MBK_G_FIXUP
#undef MBK_G_LOOP
#undef MBK_G_GROUP8
#undef MBK_G_LOOP8
#undef MBK_G_T2T4
#undef MBK_G_GROUP16
#undef MBK_G_LOOP16
#undef MBK_G_T2T7
#undef MBK_G_GROUP32
#undef MBK_G_LOOP32
#undef MBK_G_LOOP8X
#undef MBK_G_LOOP16X
#undef MBK_G_LOOP8C
#undef MBK_G_LOOP16C
#undef MBK_G_LOOP8CX
#undef MBK_G_LOOP8CXI
#undef MBK_G_LOOP8C_W
#undef MBK_G_CYC_INIT_W
#undef MBK_G_LOOP16CX
#undef MBK_G_LOOP8C_NF
#undef MBK_G_LOOP16C_NF
#undef MBK_G_LOOP8C_R
#undef MBK_G_LOOP16C_R
#undef MBK_G_LOOP8_NF
#undef MBK_G_LOOP16_NF
#undef MBK_G_CYC_INIT
#undef MBK_G_CYC
#undef MBK_G_CYC_OOL
