/*
 * mbk.h -- C ABI of libmbk_hip.so, the MI355X (gfx950) Mandelbrot tile kernel library.
 *
 * The reference (ofsouzap/DistributedMandelbrot) has NO in-process plugin / FFI interface: its only
 * compute path is a numba-CUDA ufunc inside a Python worker script.  The seam a drop-in must honour
 * is the worker<->Distributer TCP protocol (spoken by distributedmandelbrot_amd/worker.py); the
 * in-process seam is the worker's `process_workload(level, mrd, index_real, index_imag)`.  Each entry
 * point below names the reference code it replaces.  Paths are relative to the reference root;
 * "WorkerCUDA.py" = DistributedMandelbrotWorkerCUDA/DistributedMandelbrotWorkerCUDA.py.
 *
 * Conventions: plain C symbols; every call returns an int status (MBK_OK == 0); no exceptions, no
 * C++ or torch types cross the boundary; output buffers are caller-owned; one mbk_ctx per GPU; a
 * ctx is NOT thread-safe (use one host thread per ctx -- ctypes releases the GIL during calls).
 * There is NO CPU fallback: without a usable gfx950 device mbk_create fails with MBK_ERR_NO_DEVICE.
 *
 * Arithmetic contract: IEEE-754 binary64, every operation individually
 * rounded, no FMA contraction of the reference's expressions; iteration counts are bit-identical to
 * a strict evaluation of WorkerCUDA.py:39-68 on coordinates bit-identical to np.linspace's.
 */
#ifndef MBK_H
#define MBK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBK_ABI_VERSION 5

/* DataChunk.cs:20 (dataChunkRange), WorkerCUDA.py:80 (definition = 4096). */
#define MBK_CHUNK_DEFINITION 4096u
/* DataChunk.cs:27 (dataChunkSize): bytes in one tile result on the wire (Distributer.cs:415-416). */
#define MBK_CHUNK_BYTES (4096u * 4096u)

enum mbk_status {
    MBK_OK = 0,
    MBK_ERR_INVALID = 1,   /* bad argument (NULL pointer, empty window outside the view, mrd > INT32_MAX ...) */
    MBK_ERR_NO_DEVICE = 2, /* no HIP device / device index out of range / not a gfx950-class GPU */
    MBK_ERR_HIP = 3,       /* a HIP runtime call failed; see mbk_last_error */
    MBK_ERR_NOMEM = 4,
    MBK_ERR_NET = 5        /* mbk_worker_run / mbk_feeder_run: a socket call failed or the server spoke out of protocol */
};

/* flags for the compute calls */
#define MBK_WANT_COUNTS 0x1u /* write int32 escape indices (what calc_mb_value returns, WorkerCUDA.py:39) */
#define MBK_WANT_BYTES 0x2u  /* write the quantised uint8 (WorkerCUDA.py:96-98) -- fused on device */
/* Kernel selection (bits 8..11).  0 = default: "scan" or "group", decided per launch from a 256-pixel host probe of
 * the window (MBK_OPT_HEAVY_SHARE) -- a deterministic function of the window, not of earlier launches.  The others
 * exist so that the parity tests and bench.py can A/B every shipped kernel variant; all of them are bit-exact. */
#define MBK_KERNEL_SHIFT 8
#define MBK_KERNEL_MASK 0xF00u
#define MBK_KERNEL_DEFAULT 0x000u
#define MBK_KERNEL_SIMPLE 0x100u /* one lane per pixel, compiler-scheduled loop, literal (2*zr)*zi form */
#define MBK_KERNEL_ASM 0x200u    /* one lane per pixel, hand-scheduled gfx950 loop */
#define MBK_KERNEL_REFILL 0x300u /* persistent waves with lane refill (deep-zoom divergence) */
#define MBK_KERNEL_GROUP 0x400u  /* hand-scheduled loop, bailout tested once per 16 (interior) / 8 steps + exact replay; one workgroup per 8x8 block */
#define MBK_KERNEL_SCAN 0x500u   /* a persistent light pass that finishes every block whose pixels escape within 4 steps,
                                    then one workgroup (the "group" code) per block it listed as unfinished */

/* Arithmetic of the escape loop (bit 12).  Default = IEEE binary64, the reference's arithmetic.
 * MBK_PRECISION_F32 is BASELINE config 4's "fp32 kernel variant" -- NOT in the reference (its only
 * signature is int32(float64, float64, int32), WorkerCUDA.py:39): coordinates are generated in fp64
 * exactly as above, rounded once to binary32, and the loop runs in strict (contraction-free) binary32.
 * Its oracle is oracle/mandel_oracle.c:mbo_escape_f32.  Supported by the asm / group kernels. */
#define MBK_PRECISION_F32 0x1000u

/* Host-buffer calls with MBK_WANT_BYTES (bit 13): copy the quantised bytes to the host only if the tile is not
 * uniform.  The stats reduction runs on the device anyway; when it reports all_bytes_zero ("Never",
 * DataChunk.cs:82) or all_bytes_one ("Immediate", :87) the 16 MiB copy is skipped and h_bytes is left
 * UNTOUCHED -- the caller takes the constant from mbk_stats.  3 tiles in 4 of a pyramid level are of that
 * kind, and the copy (0.31 ms pinned) is 5x their kernel time.  Honoured by mbk_view_compute,
 * mbk_view_submit and mbk_datachunk_submit_ex; the decision is made in mbk_wait. */
#define MBK_LAZY_UNIFORM 0x2000u

typedef struct mbk_ctx mbk_ctx;

/*
 * A view: width x height samples of [start_r, start_r+range_r] x [start_i, start_i+range_i], both
 * endpoints included -- exactly gen_arrays' two np.linspace calls (WorkerCUDA.py:24-32) with
 * `definition` generalised to width/height.  The window (col0,row0,ncols,nrows) selects which
 * samples are computed (row bands are the multi-GPU shard unit); coordinates always come from the
 * FULL view's linspace, so a banded view is bit-identical to the whole one.
 * Output layout: element (row-row0)*ncols + (col-col0); real is the fast axis (np.tile, :34),
 * imaginary the slow one (np.repeat, :35); row 0 is start_i.
 *
 * Limits (tests/test_geometry_limits.py, tests/test_gpu_geometry_limits.py, tests/test_gpu_large_outputs.py; the
 * thresholds between the launch forms: DESIGN.md, "Geometric thresholds"):
 *   samples per axis   width, height <= 2^32 - 1: a sample index is a uint32_t and is converted to binary64 as an
 *                      unsigned number, exactly; col0 + ncols <= width and row0 + nrows <= height are checked in 64 bits.
 *   pixels per window  ncols * nrows <= 2^31.  Protects the 32-bit lane offset the kernels add to a block's 64-bit base
 *                      (at most 7 rows of the window, so below 2^31 elements), the block count (at most 2^25 blocks of
 *                      8 x 8 pixels, a 32-bit grid) and the statistics (pixel_iterations < 2^62).  An output may well be
 *                      larger than 2^32 BYTES (int32 counts of more than 2^30 pixels, float64 of more than 2^29): element
 *                      offsets are 64-bit, or a 64-bit base plus a 32-bit offset that the kernel keeps below 2^32.
 *   renders            width * s and height * s <= 2^32 - 1 for supersample s: the samples of a render are those of the
 *                      view with s times as many samples per axis, and their indices must be uint32_t as well.
 *   adaptive renders   the renders' limits; the base samples (s = 1) answer to the pixel limit for the output window, not for
 *                      the whole view: a small window of a view of more than 2^31 pixels is served.
 *   host resolve twins width * s and height * s < 2^31 for mbk_render_resolve_host, its equalized form and the adaptive
 *                      resolve twins: they take whole sample arrays on the host, indexed in 64 bits from 31-bit sizes.
 *   coordinates        finite, |x| <= 2^500 (MBK_PRECISION_F32: 2^60) for the start, the range and their sum: no inf - inf
 *                      before the bailout test.
 */
typedef struct mbk_view {
    double start_r, start_i;
    double range_r, range_i;
    uint32_t width, height;
    uint32_t col0, row0, ncols, nrows;
} mbk_view;

typedef struct mbk_stats {
    float kernel_ms;           /* hipEvent time of the escape-time kernel launch(es) on the slot's stream.  With
                                  MBK_OPT_PREPASS_OVERLAP = 1 (the default) the dispatch-order pre-pass (~13 us: a fill +
                                  classify_blocks_kernel) runs on an auxiliary stream beside the previous tile and is NOT
                                  inside this interval unless the tile kernel had to wait for it; with 0 it is */
    float d2h_ms;              /* hipEvent time of the device->host copies */
    uint64_t pixel_iterations; /* sum over pixels of (count if count>0 else mrd-1), from the kernel's own counts: the
                                  REFERENCE's iterations for this output (with the cycle test on, fewer are executed) */
    uint64_t never_pixels;     /* pixels with count == 0 (never escaped) */
    uint32_t all_bytes_zero;   /* 1 iff every quantised byte == 0: DataChunk.IsNeverChunk,     DataChunk.cs:82 */
    uint32_t all_bytes_one;    /* 1 iff every quantised byte == 1: DataChunk.IsImmediateChunk, DataChunk.cs:87 */
    uint64_t rle_runs;         /* runs of equal bytes in the quantised tile: the RLE codec (DataChunkSerializer.cs:56-100)
                                  writes 5 bytes per run, so its size is 1 + 5*rle_runs vs 1 + n for Raw (0 if no bytes) */
} mbk_stats;

typedef struct mbk_device_info {
    char name[128];
    char arch[64];
    int compute_units;
    int clock_mhz;       /* max engine clock */
    int wavefront_size;
    uint64_t total_mem;
} mbk_device_info;

int mbk_abi_version(void);

/* Number of HIP devices visible to this process. */
int mbk_device_count(int *count);

/* One context per GPU: device selection, a private stream, events, grow-on-demand device buffers.
 * Replaces the implicit default-CUDA-device context numba creates at WorkerCUDA.py:87. */
int mbk_create(int device, mbk_ctx **out);
void mbk_destroy(mbk_ctx *ctx);

/* Message for the last failing call on this ctx (ctx may be NULL for mbk_create failures).
 * The string stays valid until the next call on the same ctx / thread. */
const char *mbk_last_error(const mbk_ctx *ctx);

int mbk_get_device_info(mbk_ctx *ctx, mbk_device_info *info);
/* PCI bus id of the ctx's GPU as "dddd:bb:dd.f" (hipDeviceGetPCIBusId); len >= 16.  What a multi-GPU job reports
 * per rank so that a reader can tell N distinct GPUs took part (there is no RCCL communicator to ask). */
int mbk_device_pci_bus_id(mbk_ctx *ctx, char *buf, int len);

/* Pinned host memory for result buffers (direct DMA target of the D2H copy).  Optional: any host
 * pointer is accepted by the compute calls. */
int mbk_host_alloc(mbk_ctx *ctx, uint64_t bytes, void **out);
int mbk_host_free(mbk_ctx *ctx, void *ptr);

/* Tile geometry: WorkerCUDA.py:75-78 == DataChunk.cs:32-33,59-66.
 * range = 4/level; start = -2 + range*index (each operation individually rounded).
 * MBK_ERR_INVALID if level == 0 or an index >= level (DataChunk.cs:99-106). */
int mbk_datachunk_geometry(uint32_t level, uint32_t index_real, uint32_t index_imag,
                           double *start_r, double *start_i, double *range);

/*
 * Asynchronous launch on DEVICE pointers, on the caller's HIP stream (a hipStream_t; NULL = HIP's null
 * stream, which is what PyTorch's default stream is -- NOT the ctx's private stream).
 * Replaces gen_arrays (WorkerCUDA.py:19-37: coordinates are generated in-kernel), the two H2D copies
 * (:87-88), the ufunc launch `calc_mb_value(r_device, i_device, mrd, out=out_device)` (:92) and,
 * with MBK_WANT_BYTES, the host quantiser (:96-98).  d_counts: int32[nrows*ncols] (or NULL without
 * MBK_WANT_COUNTS); d_bytes: uint8[nrows*ncols] (or NULL without MBK_WANT_BYTES).
 * mrd is the reference's "maximum recursion depth": at most mrd-1 updates, result in {0} U [1, mrd-1].
 * A launch may enqueue helper kernels (scan pass, dispatch-order pre-pass, work-queue reset) that use
 * scratch memory the ctx keeps PER STREAM (a few bytes per 8x8 block of the largest window seen on that
 * stream): launches on one stream are ordered, so any number may be queued, on any number of streams.
 */
int mbk_view_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                    int32_t *d_counts, uint8_t *d_bytes, void *hip_stream);

/*
 * Graph capture.  Every *_launch form of this header that works on DEVICE pointers alone may be called while its stream
 * captures a graph (hipStreamBeginCapture in any mode, torch.cuda.graph), and the graph may be replayed any number of times:
 * mbk_view_launch, _launch_smooth, _launch_distance, _launch_normal and mbk_view_interior_launch; the mbk_julia_view_*, the
 * mbk_deep_view_* and the mbk_deep_xview_* launches (counts, smooth values, distance with and without a table, normals,
 * nucleus); every *_render_launch, *_render_equalized_launch, *_render_adaptive_launch, *_relief_render_launch and
 * *_distance*_render_launch, mbk_view_interior_render_launch and mbk_density_render_launch; the *_histogram_launch calls,
 * mbk_counts_histogram and mbk_view_density_launch (these three ADD into the caller's table: n replays add n times).
 * tests/test_gpu_graph.py captures and replays each of them; DESIGN.md "Graph capture" has what each enqueues.
 *
 * Inside a capture a call asks the stream for its status once (hipStreamIsCapturing) and then
 *   - enqueues everything on the caller's stream, in order: the graph is one chain without branches.  The dispatch-order
 *     pre-pass runs as under MBK_OPT_PREPASS_OVERLAP = 0 whatever the option says, into a list that only captured launches of
 *     this stream use; the ctx' auxiliary stream, its events and the option's bookkeeping are not touched;
 *   - takes MBK_OPT_XCD_BALANCE = 1 for 0 (the time stamps belong to one enqueue) and runs without the SPILL second pass;
 *   - serves MBK_KERNEL_DEFAULT at every window size -- with "group" where it would take the two-pass form of "scan" outside a
 *     capture -- and MBK_KERNEL_GROUP, _ASM and _SIMPLE as always.  Every selector stores the same counts, bytes and values, so
 *     a replay stores what the call outside the capture stores, bit for bit;
 *   - never synchronises, allocates, frees, copies synchronously or builds a table.  A call that would have to returns
 *     MBK_ERR_INVALID with a message that begins "graph capture:" BEFORE it has allocated or enqueued anything: the caller's
 *     capture stays valid, nothing is written, and the same call outside a capture succeeds.
 *
 * The warm-up rule.  What a captured call needs must already be there: make THE SAME CALL once outside a capture, on the same
 * stream of the same ctx, with the same palette (and equalisation table), the same orbit and flags, and the same view and window
 * or larger ones.  Refused inside a capture, each in its own words: the first call of a ctx on a stream; a window, a band or a
 * view for which the stream's scratch (dispatch lists, count, render and density scratch) would have to grow; a palette or an
 * equalisation table that differs from the one the stream's last render uploaded; an orbit whose copy (extended-range views: whose
 * wide table) is not on the device; an MBK_DEEP_BLA / MBK_DEEP_XBLA view whose dcmax has no resident table; an "order 3" launch
 * whose pre-pass counters were never cleared; MBK_KERNEL_SCAN and MBK_KERNEL_REFILL (their cursors and queues alternate or
 * are sized per enqueue).  Never capturable, and refused in the same way: mbk_chunk_decode_launch and mbk_chunk_render_launch
 * (they read HOST input at enqueue time), mbk_density_max and mbk_reduce_counts (they wait for their result).  The slot forms
 * (*_submit, mbk_wait) and every *_compute form run on streams of the ctx' own and take no stream to capture.
 *
 * Replays.  A captured launch holds pointers into the scratch of its (ctx, stream) and into the ctx' orbit copies and tables, so
 *   - a replay must be ORDERED against every other piece of work of the same ctx on the capture stream -- replay it on that
 *     stream, or behind an event of it -- as two launches on one stream are;
 *   - the graph stays valid until one of these calls is made on the ctx, and must not be replayed afterwards: a call on the
 *     capture stream whose scratch need is larger than any before it (the scratch is freed and allocated anew); for a graph
 *     that holds a render, a render on the capture stream with another palette or equalisation table (the stream's device copy
 *     is overwritten in place: a replay would colour through the new one); a launch that
 *     brings a THIRD dcmax to an orbit the graph uses with MBK_DEEP_BLA / MBK_DEEP_XBLA (the table asked for least recently is
 *     overwritten); the use of a NINTH orbit (all copies are dropped); a launch on a 65th stream (all scratch is dropped);
 *     mbk_destroy.  The library cannot see a graph and does not check this.
 */

/*
 * Streams.  Every *_launch form takes the caller's stream, and one ctx may have launches queued on any number of streams at
 * once, from ONE host thread at a time (a ctx is not thread-safe).  tests/test_gpu_streams.py runs every form beside the others
 * on 4 and on 12 streams, with the launches held back on the device so that they do overlap; DESIGN.md "Streams" has the table.
 *
 * Kept per (ctx, stream), made on the stream's first call and grown on demand: the dispatch lists with their pre-pass stream
 * and events, the scan cursors and lists, the SPILL buffers, the sample scratch of renders, histograms and density views, the
 * count scratch of the two-pass calls, the palette and the equalisation table of the last render, the density band counters,
 * the chunk scratch, the XCD shares.  Two launches on different streams share none of it.  The ctx' own streams (the slots of
 * *_submit and of the *_compute forms) take entries of the same table when a call on them needs scratch.
 *
 * A WARM launch form -- same or smaller window, same palette and table, resident orbit and dcmax -- enqueues and returns: it
 * waits for nothing, whatever is queued on its stream or on others.  What does wait, and for what:
 *   - the caller's stream (and the stream's pre-pass stream): dispatch lists, scan lists or SPILL buffers that must grow; the
 *     first "order 3" launch of a stream; a change of MBK_OPT_PREPASS_OVERLAP since the stream's last ordered launch; a render
 *     whose palette or equalisation table differs from the stream's last (the device copy is overwritten in place, behind the
 *     renders that read it); mbk_density_max, mbk_reduce_counts, MBK_INFO_SPILL;
 *   - the whole DEVICE, every stream of every ctx and of the caller's own work included: sample or count scratch that must grow
 *     (the old buffer is freed, and hipFree waits for the device); an MBK_DEEP_BLA / MBK_DEEP_XBLA launch whose dcmax is not
 *     resident while both places beside the orbit are taken (the table asked for least recently is overwritten; an adaptive
 *     render keeps both of its own); the use of a NINTH orbit on a ctx that holds eight copies (all eight are freed); the first
 *     call on a stream when the table already holds 64 streams, the ctx' own among them (the scratch of all 64 is freed and
 *     made anew as the streams come back; a stream's palette and table are then uploaded again); mbk_destroy.
 * A first call on a stream, an orbit's first launch and a table into a free place allocate and copy synchronously; the library
 * waits for no launch there, and they may be made beside queued work of other streams.  Whether hipMalloc or a synchronous
 * hipMemcpy waits for queued work is the runtime's to say: in the tests it did not, but for one such call in some thirty
 * (profiles/streams/README.md).  The *_compute forms wait for their own result, and like any call they drain the device where
 * one of the ctx' buffers must grow.
 * A caller that creates streams without end pays the 64-stream drain again and again: keep a pool (PyTorch's holds 32 streams
 * per priority).  Accumulating forms (the *_histogram_launch calls, mbk_counts_histogram, mbk_view_density_launch) add with
 * device-wide atomics: any number of streams may add into one table, and the table holds the sum.
 */

/* Synchronous: launch + D2H into HOST buffers (either may be NULL according to flags) + stats.
 * Replaces WorkerCUDA.py:82-98 for a generic view. */
int mbk_view_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                     int32_t *h_counts, uint8_t *h_bytes, mbk_stats *stats);

/* Synchronous: one 4096x4096 DataChunk tile, exactly the reference's
 * `process_workload(level, mrd, index_real, index_imag) -> uint8[16777216]` (WorkerCUDA.py:70-100).
 * h_bytes: MBK_CHUNK_BYTES bytes, the payload the worker sends after 0x20 (WorkerCUDA.py:168).
 * h_counts: optional int32[16777216] (NULL to skip its D2H). */
int mbk_datachunk(mbk_ctx *ctx, uint32_t level, uint32_t mrd, uint32_t index_real,
                  uint32_t index_imag, uint8_t *h_bytes, int32_t *h_counts, mbk_stats *stats);

/*
 * BASELINE config 5 -- continuous ("smooth") escape-time colouring.  NOT in the reference (its output
 * is the integer index quantised to a byte, WorkerCUDA.py:96-98); defined here as
 *     nu = n + 1 - log2(0.5 * ln |z_n|^2)   for a pixel that escapes at step n (|z_n|^2 >= 4 is the
 *                                            reference's own bailout value), and 0 if it never escapes,
 * in binary64.  n is the bit-exact count of the parity kernels (also returned) and |z_n|^2 the binary64 value that
 * tripped the test, every operation rounded on its own; the logarithms are the device's (ocml).  Against the
 * correctly rounded value of the formula at that |z_n|^2 the tests allow A ulp(nu) + B 2^-52 with A = 2.57, B = 3.38:
 * glibc's libm measures A0 = 1.57, B0 = 1.38 on the same cases (A where |nu| >= 1, B where |nu| < 1, both worst at
 * n = 1 with |c| ~ 50), and the device gets one more ulp(nu) and two more 2^-52.  Measured on gfx950:
 * A = 1.570 at n = 1, |z_1|^2 = 11337031.25 and B = 1.379 at n = 1, |z_1|^2 = 75820.85571289062, the same pixels and
 * digits as glibc; over cfg5 at full size the worst sampled pixel is 1.195 ulp(nu) (n = 1, |z_1|^2 = 18.177277466062407).
 * When |z_n|^2 overflows binary64 (possible at n = 1 only, for |c| above ~1e77) nu is -inf, the limit of the formula
 * and what IEEE logarithms return; it is never NaN.  mrd 0 and 1 run no step: every count and nu is 0.
 * Asynchronous form on DEVICE pointers / caller's stream (window-sized buffers, ncols * nrows elements, nothing is
 * written outside them), and synchronous form into HOST buffers.  d_counts / h_counts may be NULL.  MBK_ERR_INVALID,
 * with nothing written: NULL d_smooth / h_smooth, MBK_PRECISION_F32 in the flags of _launch_smooth (there is no
 * binary32 form; _compute_smooth ignores every flag but the kernel), the kernels MBK_KERNEL_SIMPLE and
 * MBK_KERNEL_REFILL, mrd >= 2^31, and whatever mbk_view_launch refuses in a view.
 */
int mbk_view_launch_smooth(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                           int32_t *d_counts, double *d_smooth, void *hip_stream);
int mbk_view_compute_smooth(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                            int32_t *h_counts, double *h_smooth, mbk_stats *stats);

/*
 * Exterior distance estimates for plain views.  NOT in the reference; additive (the ABI version stays 5): no existing call
 * changes.  The derivative d = dz/dc is carried along the orbit and the pixel reports
 *     de = 2 |z| ln |z| / |d|,
 * a length in the complex plane within a known factor of the true distance from c to the set (for a point outside, the
 * distance lies between de / 4 and about de; Koebe's quarter theorem gives de <= 4 x distance).
 *
 * Contract (tests/distance_model.py restates it in numpy; tests/test_gpu_distance.py holds the GPU to it).  For a pixel with
 * coordinate c = (cr, ci) of a view (the linspace of mbk_view), binary64, every operation rounded on its own:
 *   state     z_0 = c, d_0 = (1, 0).  Step k -> k + 1, for the same steps the count loop runs (at most mrd - 1 updates):
 *               u = fl(fl(zr dr) - fl(zi di)), v = fl(fl(zr di) + fl(zi dr))   both from z_k and d_k
 *               dr' = fl(2u + 1), di' = 2v      (2u and 2v are exact, subnormals included, so fma(u, 2, 1) IS fl(2u + 1); where 2u
 *                                                overflows, fl(2u + 1) and fl(fl(2u) + 1) are the same infinity: no case differs)
 *               z_(k+1) by the recurrence of mbk_view_launch, unchanged.
 *   count     n is exactly the count of mbk_view_launch (first k with |z_k|^2 >= 4, 0 if none; c is never tested).
 *   run-on    a pixel with n > 0 runs on, uncounted, with the same two recurrences until mag = fl(fl(zr^2) + fl(zi^2)) >= 2^32 or
 *             64 further steps have run, whichever comes first (these steps may go past mrd - 1; n does not change).  At the
 *             reference's bailout radius 2 the formula is useless near the set: on c = -2 - t it reads 12 to 9e5 times the
 *             true distance t at the step that trips `>= 4`, and 3.885 t .. 4 t at 2^32.  Next to c = -2 the excess over
 *             |z| = 2 only triples per step (13 further steps at t = 1e-6, ~34 at 1e-16), hence 64 and not 8.
 *   output    de = fl(fl(sqrt(fl(mag / dmag))) fl(ln mag)), dmag = fl(fl(dr^2) + fl(di^2)), at the final state; 0 if n = 0.
 *             ln is the device's (ocml); division and square root are the correctly rounded ones.  Against the correctly rounded
 *             value of the expression at (mag, dmag) the tests allow the host (glibc) what tests/distance_model.py measures,
 *             and the device one ulp more.
 *   special   never NaN: where the expression is NaN (mag = dmag = inf; a NaN in d after inf - inf) 0 is stored.  Infinities are
 *             stored as IEEE arithmetic gives them: mag = inf (|c| above ~1e77, n = 1) gives +inf; an overflowed dmag with a
 *             finite mag gives 0; dmag = 0 gives +inf.  c = -2 itself (n = 1, z stays at 2 through the run-on) is finite.
 *   mrd       0 and 1 run no step: every count and de is 0.
 * Windows of a view are bit-identical to the whole view.
 *
 * Two designs are built in, selected by the kernel bits of `flags`, bit-identical in what they store:
 *   MBK_KERNEL_DEFAULT / _SCAN / _GROUP   two passes: mbk_view_launch with that selector writes the counts (cycle test and all:
 *             it retires the interior, which needs no derivative), then a derivative pass runs each pixel with n > 0 for exactly
 *             n steps without a bailout test, plus the run-on.  With d_counts == NULL the counts live in scratch the ctx keeps
 *             per stream (4 bytes per pixel of the largest such window).
 *   MBK_KERNEL_ASM                        one pass: the derivative rides in a per-step escape loop; no counts are read.
 * Asynchronous form on DEVICE pointers / caller's stream (window-sized buffers, nothing is written outside them) and synchronous
 * form into HOST buffers on slot 0 (the slot-0 rule below applies; stats as for mbk_view_compute_smooth: pixel_iterations counts
 * the reference's iterations, the run-on steps are not in it).  d_counts / h_counts may be NULL.  MBK_ERR_INVALID, with nothing
 * written: NULL d_distance / h_distance, MBK_PRECISION_F32 in the flags of _launch_distance (there is no binary32 form;
 * _compute_distance ignores every flag but the kernel), MBK_KERNEL_SIMPLE and MBK_KERNEL_REFILL, mrd >= 2^31, and whatever
 * mbk_view_launch refuses in a view.  Deep views have a form of their own, with a derivative whose exponent cannot overflow
 * and the view's span as the unit: mbk_deep_view_launch_distance, below ("Distance estimates for deep views").
 */
int mbk_view_launch_distance(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                             int32_t *d_counts, double *d_distance, void *hip_stream);
int mbk_view_compute_distance(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                              int32_t *h_counts, double *h_distance, mbk_stats *stats);
/* "output" and "special" above on the HOST, compiled from the function the kernel uses (with the host's ln): no ctx, no
 * device.  For the CPU tests. */
double mbk_distance_value_host(double mag, double dmag, int32_t count);

/* NOTE on slot 0: the synchronous calls (mbk_view_compute, mbk_datachunk, mbk_view_compute_smooth,
 * mbk_quantise_counts) and mbk_serialize_last work on slot 0's buffers; while a tile submitted on slot 0 has not
 * been waited for they return MBK_ERR_INVALID instead of touching them. */
/*
 * Several tiles in flight per context (each slot has its own HIP stream, events and device buffers, allocated on first
 * use: the D2H of one tile overlaps the kernels of the others, and the host's per-tile work -- enqueue, wake-up -- hides
 * behind the GPU's).  mbk_datachunk_submit enqueues kernel + stats reduction + D2H for a tile on `slot`
 * (0 .. MBK_SLOTS-1) and returns at once; mbk_wait blocks until that slot's tile is in h_bytes / h_counts (use pinned
 * memory, mbk_host_alloc, or the copy is not asynchronous) and fills stats.  A slot holds one tile at a time.  Slot 0 is
 * also what the synchronous calls use.  Same single-host-thread rule as everything else on a ctx.  Two slots were
 * round 1-4's pipeline (1 973 tiles/s on level 16 against a bound of 2 490: every wait exposed the host's enqueue +
 * wake-up latency); four keep the copy engine and the CUs fed (profiles/r05).
 *
 * MBK_LAZY_UNIFORM (flags of mbk_datachunk_submit_ex / mbk_view_submit): the caller does not need h_bytes when the tile
 * turns out uniform (stats.all_bytes_zero / all_bytes_one: DataChunk.cs:82,87 "Never" / "Immediate" chunks, which the
 * server stores without a payload).  Then (1) a window that lies wholly outside |c| = 2 (with a margin of 1e-8) is
 * answered on the host without any GPU work when mrd >= 256: every count is 1, every byte 1 (proof:
 * tests/test_oracle.py) -- the corners of [-2, 2]^2 outside the inscribed circle, 1 - pi/4 = 21 % of the tiles of a deep
 * pyramid level (32 of level 16's 256; its other 160 "Immediate" tiles hold counts 1..4 and are computed); (2) the copy of a tile whose host probe says "all gone within 4 steps" is decided when the
 * statistics arrive; (3) every other tile is copied as usual.  h_bytes of a tile reported uniform is unspecified.
 */
#define MBK_SLOTS 4
/* Tiles the worker loops (mbk_worker_run, worker.run_pipelined) keep in flight on one ctx: the measured-best depth of the
 * host-buffer pipeline (profiles/r05/level16.log: level 16 at 2 / 3 / 4 in flight = 2 235 / 2 326 / 2 262 tiles/s, with
 * MBK_LAZY_UNIFORM 4 400 / 4 603 / 4 331); MBK_SLOTS is the capacity a caller of mbk_*_submit may use. */
#define MBK_WORKER_DEPTH 3
int mbk_datachunk_submit(mbk_ctx *ctx, int slot, uint32_t level, uint32_t mrd, uint32_t index_real,
                         uint32_t index_imag, uint8_t *h_bytes, int32_t *h_counts);
int mbk_datachunk_submit_ex(mbk_ctx *ctx, int slot, uint32_t level, uint32_t mrd, uint32_t index_real,
                            uint32_t index_imag, uint8_t *h_bytes, int32_t *h_counts, uint32_t flags /* MBK_LAZY_UNIFORM */);
int mbk_wait(mbk_ctx *ctx, int slot, mbk_stats *stats);
/* The host-side test behind MBK_LAZY_UNIFORM's short cut, without a device or a context: *outside = 1 when every sample
 * of the window has |c|^2 >= 4 (1 + m), m = 1e-8 (1e-4 with MBK_PRECISION_F32 in flags) -- then calc_mb_value returns 1
 * for every pixel when mrd >= 2 (WorkerCUDA.py:54-63: z1 = c^2 + c, |z1| >= |c| (|c| - 1) > 2).  For the CPU tests. */
int mbk_view_outside_circle(const mbk_view *view, uint32_t flags, int *outside);
/* Likewise: *literal = 1 when the window holds a row whose imaginary coordinate is non-zero but below 2^-900 (2^-100 in
 * binary32) -- the one case in which fma(2, zr * zi, ci) differs from the reference's fl(fl((2 * zr) * zi) + ci) (a
 * subnormal product), so that the launch takes the kernels with the literal form.  For the CPU tests. */
int mbk_view_needs_literal_doubling(const mbk_view *view, uint32_t flags, int *literal);
/* The same for a generic view / window (the multi-GPU shard unit is a row band of a view): enqueue on
 * `slot`, results land in h_counts / h_bytes (either may be NULL according to flags) after mbk_wait. */
int mbk_view_submit(mbk_ctx *ctx, int slot, const mbk_view *view, uint32_t mrd, uint32_t flags,
                    int32_t *h_counts, uint8_t *h_bytes);

/*
 * Deep-zoom views (ABI 5; NOT in the reference): perturbation with rebasing.  A view's pixels above are np.linspace samples
 * in binary64, which stop being distinct below a span of ~1e-13 around |c| ~ 1.  A deep view instead names its centre C as a
 * decimal string, computes one reference orbit of C in fixed point on the host, and iterates every pixel's OFFSET from it in
 * binary64 on the GPU.  DataChunk tiles, the worker protocol and the mbk_view_* calls are untouched (a tile's pixel step is
 * >= 4 / (2^32 * 4095), ~1000 ulps at |c| ~ 1.5).
 *
 * Contract (bit-exact; tests/deep_model.py restates it in numpy, tests/test_gpu_deep.py holds the GPU to it):
 *   reference orbit  C parsed from [+-]?digits[.digits]?([eE][+-]?digits)? as sign * floor(|C| 2^P) / 2^P (P fraction
 *                    bits, 64 <= P <= 4096, a multiple of 64; |Cr|, |Ci| < 4).  Z_0 = 0, Z_{k+1} = Z_k^2 + C in fixed
 *                    point, every product truncated toward zero to P bits; stop at the first M with |Z_M|^2 >= 4 (of the
 *                    truncated squares), or at M = the orbit's mrd.  Z_0 .. Z_M are stored rounded to nearest binary64.
 *   pixel offsets    column k of a view of width W and span R_r: dc_r = fl(fl(k - (W-1)/2) * s_r), s_r = fl(R_r / (W-1));
 *                    dc_r = 0 for W = 1; rows likewise.  A window's offsets come from the full view, so a band is
 *                    bit-identical to the same rows of the whole view.  Row 0 is the lowest imaginary part, as for mbk_view.
 *   step             dz = dc, m = 1 (if M == 1: dz = fl(Z_1 + dc), m = 0).  For i = 1 .. mrd-1, every operation
 *                    individually rounded, no contraction:
 *                      ar = fl(2 Z_m.r + dz.r); ai = fl(2 Z_m.i + dz.i)
 *                      dz = (fl(fl(fl(ar dz.r) - fl(ai dz.i)) + dc.r), fl(fl(fl(ar dz.i) + fl(ai dz.r)) + dc.i)); m = m + 1
 *                      z = (fl(Z_m.r + dz.r), fl(Z_m.i + dz.i)); mag = fl(fl(z.r z.r) + fl(z.i z.i))
 *                      mag >= 4: count = i, stop
 *                      mag < fl(fl(dz.r dz.r) + fl(dz.i dz.i)) or m == M: dz = z, m = 0
 *                    count 0 if the pixel never escapes -- calc_mb_value's convention (z starts at c, c is never tested),
 *                    so bytes are the usual quantiser of the count and smooth = n + 1 - log2(0.5 ln mag) as for mbk_view.
 * Limits: spans (range_r, range_i) in [2^-960, 4] (binary64 offsets stay normal); P <= 4096 (spans below 2^(64-P) resolve the
 * centre more finely than the orbit does: Python's DeepOrbit picks P = 64 + ceil(-log2 min_span) by default); a launch's mrd
 * <= the orbit's mrd.  Spans below 2^-960 take a view struct and a kernel of their own (mbk_deep_xview, "Extended-range deep
 * views" below: offsets and orbit carry an int32 exponent); series approximation is a flag (MBK_DEEP_BLA, "Deep-zoom views
 * with bilinear approximation" below), off by default.
 * Centres within ~1e-16 of -2 render wrong below spans of ~1e-15: the real orbit stays just inside |z| = 2, the binary64 table
 * holds 2.0, and every pixel retires at count 1 (tests/test_deep_truth.py, the strict xfail cases).
 *
 * An orbit is read-only after mbk_deep_orbit_create and may be used by any number of ctxs on any threads (it needs no device
 * and no ctx).  Each ctx uploads its own device copy on the orbit's first launch there, keyed by an id that is never
 * reused: 32 bytes x (M + 1) per copy (Z and 2Z, which is exact).  A copy lives until mbk_destroy -- or until a ctx holds 8
 * copies and needs a ninth: then the ctx synchronises the device (no launch that may read a copy is left) and frees all of
 * them.  Destroying an orbit does not free its copies.  The first launch of an orbit on a ctx allocates and copies
 * synchronously: launch once before capturing deep launches into a graph ("Graph capture": inside a capture that first launch
 * is refused).
 */
typedef struct mbk_deep_orbit mbk_deep_orbit;

/* A deep view: width x height pixels centred on the orbit's C, spans range_r x range_i (end samples included); the window
 * (col0, row0, ncols, nrows) selects the pixels computed, laid out as for mbk_view. */
typedef struct mbk_deep_view {
    double range_r, range_i;
    uint32_t width, height;
    uint32_t col0, row0, ncols, nrows;
} mbk_deep_view;

/* The reference orbit of (center_r, center_i) at precision_bits fraction bits, up to mrd (>= 2).  Host only: no device, no
 * ctx.  MBK_ERR_INVALID for a malformed string, |component| >= 4, precision_bits outside {64, 128, ..., 4096}, mrd < 2. */
int mbk_deep_orbit_create(const char *center_r, const char *center_i, uint32_t precision_bits, uint32_t mrd,
                          mbk_deep_orbit **out);
void mbk_deep_orbit_destroy(mbk_deep_orbit *orbit);
/* M, whether |Z_M|^2 >= 4 (else M = mrd), P, and the orbit's mrd; any output pointer may be NULL. */
int mbk_deep_orbit_info(const mbk_deep_orbit *orbit, uint32_t *length, uint32_t *escaped, uint32_t *precision_bits,
                        uint32_t *mrd);
/* Z_0 .. Z_M as binary64 into zr[0..M], zi[0..M]; n is their capacity (MBK_ERR_INVALID below M + 1). */
int mbk_deep_orbit_read(const mbk_deep_orbit *orbit, double *zr, double *zi, uint64_t n);
/* Z_0 .. Z_M of the wide table ("Extended-range deep views", below), Z_m = (xr[m], xi[m]) 2^xe[m]; n as above. */
int mbk_deep_orbit_read_wide(const mbk_deep_orbit *orbit, double *xr, double *xi, int32_t *xe, uint64_t n);
/* The three forms of the view calls.  flags: MBK_WANT_COUNTS | MBK_WANT_BYTES, and MBK_DEEP_BLA ("Deep-zoom views with
 * bilinear approximation", below), only (kernel selection, MBK_PRECISION_F32 and MBK_LAZY_UNIFORM are MBK_ERR_INVALID), as are a NULL orbit, a view without output, ranges outside [2^-960, 4] and
 * mrd > the orbit's mrd.  _launch: DEVICE pointers on the caller's stream (d_smooth may be NULL; no statistics).  _compute:
 * synchronous into HOST buffers on slot 0 (h_smooth may be NULL), stats as for mbk_view_compute -- pixel_iterations counts
 * the reference's iterations (count, or mrd - 1 for 0).  _submit: on `slot`, completed by mbk_wait. */
int mbk_deep_view_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                         int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, void *hip_stream);
int mbk_deep_view_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd, uint32_t flags,
                          int32_t *h_counts, uint8_t *h_bytes, double *h_smooth, mbk_stats *stats);
int mbk_deep_view_submit(mbk_ctx *ctx, int slot, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                         uint32_t flags, int32_t *h_counts, uint8_t *h_bytes);

/*
 * Deep-zoom views with bilinear approximation.  NOT in the reference; additive (the ABI version stays 5): without the flag
 * every call stores what it stored before.  While a pixel's offset dz is tiny against the reference orbit, the step
 * dz -> 2 Z_m dz + dz^2 + dc is linear in (dz, dc) to working precision, and a run of 2^l such steps collapses into one map
 * dz -> A dz + B dc whose coefficients come from a table merged pairwise over the orbit (BLA, the modern form of series
 * approximation).  A deep pixel then executes a fraction of its steps (scripts/deep_bla_rate.py, profiles/deep_bla/).
 *
 * MBK_DEEP_BLA is a flag of mbk_deep_view_launch / _compute / _submit, of mbk_deep_view_render_launch / _compute and their
 * _equalized_ forms (every source but MBK_RENDER_DISTANCE_REL) and of mbk_deep_view_histogram_launch / _compute.  Every other
 * call refuses it with MBK_ERR_INVALID: the deep distance calls (the estimate that takes skips lives behind names of its own:
 * "Distance estimates for deep views with bilinear approximation", below), every plain view call and every Julia call.
 *
 * Contract (tests/deep_bla_model.py restates it in numpy; tests/test_deep_bla.py holds the host twins below to it and it to
 * the truth, tests/test_gpu_deep_bla.py holds the GPU to it, bit for bit).  Everything of "Deep-zoom views" stands: orbit
 * table, offsets dc, the step, the rebase rule, counts, bytes, smooth, statistics (pixel_iterations counts the reference's
 * iterations -- count, or mrd - 1 for 0 -- not the steps executed).  Binary64 throughout, every operation rounded on its own,
 * no contraction.
 *   table     built on the host from the orbit's binary64 table Z_0 .. Z_M and one number per view,
 *               dcmax = fl(|dc_r(column 0)| + |dc_i(row 0)|) of the FULL view, not the window
 *             (a 1-norm: nothing is squared, so it cannot underflow at span 2^-960; windows and bands share one table and stay
 *             bit-identical to the whole view), with eps = 2^-40.  Level l has n_l = floor((M - 1) / 2^l) entries, for
 *             l = 0 .. while n_l >= 1; entry j covers the 2^l steps that start at m = 1 + j 2^l.  With M <= 1 there is no
 *             table and the flag changes nothing.
 *             Level 0: A = (2 Z_m.r, 2 Z_m.i), B = (1, 0), r = fl(eps fl(sqrt(fl(fl(A_r^2) + fl(A_i^2))))).
 *             Level l + 1, entry j, from x = entry 2j and y = entry 2j + 1 of level l:
 *               A = A_y A_x;  B = A_y B_x + B_y
 *               (complex products are (fl(fl(ac) - fl(bd)), fl(fl(ad) + fl(bc))) with (a, b) the left factor; the sum is
 *               rounded per component; |A_x| and |B_x| are fl(sqrt(fl(fl(.^2) + fl(.^2)))))
 *               t = fl(fl(r_y - fl(|B_x| dcmax)) / |A_x|);  r = min(r_x, max(t, 0))
 *               r = 0 whenever |A_x| = 0 or any component of the merged A, of the merged B, or t is not finite.  High levels
 *               overflow (|A| grows like 4^(2^l)); such an entry is simply never taken.  Its A and B are stored as computed
 *               (infinities, NaNs of the host's own sign and payload).
 *             r is non-increasing in l at a fixed starting m.  Stored per entry: A, B and rc = fl(r 0.7071067811865476).
 *   step      state (dz, m, i), i the index of the step about to run.  Take the highest level l with ALL of
 *               m >= 1;  (m - 1) mod 2^l = 0;  (m - 1) >> l < n_l;  i + 2^l <= mrd;  max(|dz.r|, |dz.i|) < rc
 *             (each is monotone in l: a search upward from level 0 that stops at the first failure finds the same level).
 *             If there is one:
 *               dz = (fl(fl(fl(A_r dz.r) - fl(A_i dz.i)) + fl(fl(B_r dc.r) - fl(B_i dc.i))),
 *                     fl(fl(fl(A_r dz.i) + fl(A_i dz.r)) + fl(fl(B_r dc.i) + fl(B_i dc.r))));  m += 2^l
 *               and the step index becomes i + 2^l - 1.  If there is none, the plain step runs.  After either, exactly as in
 *             "Deep-zoom views": z = fl(Z_m + dz) and mag are formed; mag >= 4 stores that step index as the count (its mag
 *             feeds smooth); then the rebase rule applies (mag < |dz|^2 or m == M).  The steps inside a skip are not tested.
 *             m = 0, the state right after a rebase, always takes the plain step.
 *   eps       2^-40, a constant of the contract (it changes output, so it is not an mbk_option).  Against direct iteration at
 *             P + 128 bits it equals the truth on every sampled pixel of the catalogue of tests/test_deep_truth.py and of the
 *             seahorse view at span 1e-20, mrd 30000; the 2^-24 the literature suggests for binary64 reaches 88.75 % there, off
 *             by up to 140 (tests/test_deep_bla.py keeps that test).  The same cap as the plain contract: >= 99 % of pixels.
 *
 * The ctx keeps the device copies of up to two tables beside each orbit copy, keyed by the orbit's id and the bits of dcmax:
 * 40 bytes per entry, fewer than 2 (M - 1) entries each.  A table is built on the host and uploaded, synchronously, by the
 * first MBK_DEEP_BLA launch on the ctx that brings its dcmax (another span, aspect or size of the full view); once both places
 * are taken it goes over the table asked for least recently, and that first synchronises the device, since a queued launch may
 * still read the table it replaces.  So the orbit's "first launch" rule covers it: launch once per (orbit, spans) before
 * capturing, and expect three or more dcmax in turn on one orbit to serialise.  The tables are freed with the orbit copies.
 */
#define MBK_DEEP_BLA 0x8000u
/* Host twins for the CPU tests, compiled from the functions the builder and the kernel use: no ctx, no device.  `view` gives
 * dcmax (its window is not used); MBK_ERR_INVALID for what mbk_deep_view_launch refuses in a view.
 * _info: the number of levels (0 for M <= 1) and of entries over all levels.  _read: level `level` into five arrays of
 * capacity n (MBK_ERR_INVALID below n_level, or for a level the table does not have).  _count_host: the pixel (col, row) of
 * the full view under the rule above -- its count, the mag of the escaping step (0 for count 0) and the number of steps
 * executed, a skip counting as one. */
int mbk_deep_bla_info(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t *levels, uint64_t *entries);
int mbk_deep_bla_read(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t level, double *A_r, double *A_i,
                      double *B_r, double *B_i, double *rc, uint64_t n);
int mbk_deep_bla_count_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                            int32_t *count, double *mag, uint64_t *steps_executed);

/*
 * Extended-range deep views.  NOT in the reference; additive (the ABI version stays 5): no existing call changes, and what
 * the mbk_deep_view_* calls store is untouched.  A deep view above stops at spans of 2^-960 because its offsets, and the
 * orbit table it reads, are binary64: below ~1e-308 a span cannot be named, and a reference point within 1e-308 of 0 -- every
 * multiple of the period when the view looks at a small minibrot -- is subnormal or 0 in the table exactly where rebasing
 * compares |Z_m + dz| with |dz|.  An extended-range view carries every number as a binary64 mantissa pair with one int32
 * exponent, on the host (the wide table) and on the device (csrc/mbk_deep_wide.h), so spans reach as far as the fixed-point
 * orbit does: P <= 4096 fraction bits, spans down to ~2^-4030.  It covers counts, bytes, smooth values, renders (sources
 * bytes, smooth, equalized) and histograms; its distance estimates are calls of their own ("Distance estimates for
 * extended-range deep views", below) and MBK_DEEP_BLA is not implemented for it (its bilinear approximation is a flag of its
 * own: MBK_DEEP_XBLA, "Extended-range deep views with bilinear approximation", below).
 *
 * Contract (bit-exact; tests/deep_wide_model.py restates it in numpy; tests/test_deep_wide.py holds the host twins below to
 * it and it to the truth, tests/test_gpu_deep_wide.py holds the GPU to it).  Binary64 mantissas, int32 exponents, every
 * floating operation rounded on its own, no contraction.  EZ = -2^24 is the exponent of a zero.
 *   wide table   beside the binary64 table, built once by mbk_deep_orbit_create: every Z_m of the fixed-point orbit as
 *                (X_r, X_i, xe), Z_m = X 2^xe.  xe is the frexp exponent of the larger |component| taken from the fixed-point
 *                value (its bit length minus P); X_r and X_i are the fixed-point components times 2^-xe, each rounded to
 *                nearest-even binary64 (so the larger lies in [0.5, 1], 1 when it rounds up; the smaller, if it lands in the
 *                subnormal range, rounds once on that grid).  A zero Z is (0, 0, EZ).  Wherever an entry of the binary64 table
 *                is a normal number it equals X 2^xe bit for bit.
 *   view         spans range_* 2^exp2 with range_* in [2^-64, 4] and exp2 in [-8192, 0].  The offsets are dc = dcm 2^exp2 with
 *                dcm the offset formula of "Deep-zoom views" applied to range_* (column k: fl(fl(k - (W-1)/2) fl(range_r /
 *                (W-1))), 0 for W = 1), from the full view: a window is bit-identical to the same pixels of the whole view.
 *   helpers      sh(x, k) = ldexp(x, max(k, -1200)): exact unless the result is subnormal, and then it rounds once.
 *                norm(v, e): with s the frexp exponent of max(|v_r|, |v_i|), (ldexp(v_r, -s), ldexp(v_i, -s), e + s); (0, 0, EZ)
 *                when both components are 0.
 *   step         per pixel (w, q, m), dz = w 2^q.  Start (w, q) = norm(dcm, exp2), m = 1; if M == 1 that state goes through (e)
 *                with the entry 1 at once -- (w, q) = norm(zv, t), m = 0 -- as the plain contract's start does.
 *                For i = 1 .. mrd-1, with (X, xe) the entry m:
 *                  a. g = max(xe + 1, q);  A = fl(sh(X, xe + 1 - g) + sh(w, q - g)), per component
 *                  b. p = (fl(fl(A_r w_r) - fl(A_i w_i)), fl(fl(A_r w_i) + fl(A_i w_r))), exponent g + q
 *                  c. h = max(g + q, exp2);  N = fl(sh(p, g + q - h) + sh(dcm, exp2 - h))
 *                  d. (w, q) = norm(N, h);  m = m + 1
 *                  e. with (X, xe) the entry of the new m: t = max(xe, q);  zv = fl(sh(X, xe - t) + sh(w, q - t));
 *                     mg = fl(fl(zv_r^2) + fl(zv_i^2));  mag = ldexp(mg, 2 max(t, -600))
 *                  f. mag >= 4: count = i, stop (this mag feeds smooth as in "Deep-zoom views")
 *                  g. dm = fl(fl(w_r^2) + fl(w_i^2));  if mg < ldexp(dm, 2 max(q - t, -600)) or m == M: (w, q) = norm(zv, t), m = 0
 *                count 0 if the pixel never escapes; bytes are the usual quantiser; mrd 0 and 1 run no step; statistics as for
 *                mbk_deep_view_compute (pixel_iterations counts count, or mrd - 1 for 0).
 *   corners      The exponents are nominal: p and N are not renormalised between (b) and (c), so if A cancels to exactly 0
 *                while g + q exceeds exp2 by more than ~1000, sh(dcm, exp2 - h) underflows and that step adds no dc (2 Z_m
 *                = -dz exactly: no sampled pixel of the tests meets it).  A zero operand has exponent EZ, far below any other, so
 *                it never sets g, h or t unless both are zero.  All exponents stay within +-2^26.
 *   equals plain Scaling by a power of two is exact: wherever no value of the plain deep contract is subnormal or underflows,
 *                an extended-range view stores the same count and the same mag, bit for bit, as the plain view of the same
 *                spans (tests/test_deep_wide.py, on the catalogue of tests/test_deep_truth.py).
 * Against direct iteration at P + 128 bits: >= 99 % of sampled pixels equal, the cap of the plain contract, at exp2 = -1100 and
 * -3000 and on the centre 1e-400, whose binary64 table holds 0 in every entry.  Centres within ~1e-16 of -2 stay a known limit.
 *
 * Each ctx uploads its device copy of the wide table (32 bytes x (M + 1)) on the orbit's first extended-range launch there and
 * keeps it beside the orbit's binary64 copy, under the same lifetime and eviction rule; that upload is synchronous too: launch
 * once before capturing.
 */
typedef struct mbk_deep_xview {
    double range_r, range_i;   /* in [2^-64, 4] */
    int32_t exp2;              /* in [-8192, 0]: the spans are range_* 2^exp2 */
    uint32_t width, height, col0, row0, ncols, nrows;
} mbk_deep_xview;

/* The three forms, as mbk_deep_view_launch / _compute / _submit: the same outputs, flags (MBK_WANT_COUNTS | MBK_WANT_BYTES,
 * and MBK_DEEP_XBLA, only), statistics and refusals; in addition MBK_DEEP_BLA, ranges outside [2^-64, 4] and exp2 outside [-8192, 0] are
 * MBK_ERR_INVALID. */
int mbk_deep_xview_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                          int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, void *hip_stream);
int mbk_deep_xview_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd, uint32_t flags,
                           int32_t *h_counts, uint8_t *h_bytes, double *h_smooth, mbk_stats *stats);
int mbk_deep_xview_submit(mbk_ctx *ctx, int slot, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                          uint32_t flags, int32_t *h_counts, uint8_t *h_bytes);
/* Host twin for the CPU tests, compiled from the step functions the kernel uses: no ctx, no device.  The pixel (col, row) of
 * the full view: its count and the mag of the escaping step (0 for count 0).  MBK_ERR_INVALID for what the launch refuses. */
int mbk_deep_xview_count_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                              int32_t *count, double *mag);

/*
 * Extended-range deep views with bilinear approximation.  NOT in the reference; additive (the ABI version stays 5): without
 * the flag every call stores what it stored before, and MBK_DEEP_BLA keeps being refused by every mbk_deep_xview_* call.
 * Extended-range views are the ones with the largest iteration counts -- a pixel 2^-3000 from its centre runs ~2400 steps
 * that are linear to working precision before anything else happens -- and their step is the most expensive in the library.
 * The table of "Deep-zoom views with bilinear approximation" cannot serve them: its coefficients overflow binary64 (|A| grows
 * like 4^(2^l)) and every useful radius is below 1e-308.  This table carries A, B and the radius as binary64 mantissas with
 * int32 exponents, like the wide step; that also removes the overflow ceiling on the levels.
 *
 * MBK_DEEP_XBLA is a flag of mbk_deep_xview_launch / _compute / _submit, of mbk_deep_xview_render_launch / _compute and their
 * _equalized_ forms (sources bytes, smooth, equalized) and of mbk_deep_xview_histogram_launch / _compute.  Every other call
 * refuses it with MBK_ERR_INVALID and writes nothing: plain views, Julia views, mbk_deep_view_*, the distance, interior and
 * density calls.  MBK_DEEP_XBLA | MBK_DEEP_BLA is refused as MBK_DEEP_BLA alone is.
 *
 * Contract (tests/deep_wide_bla_model.py restates it in numpy; tests/test_deep_wide_bla.py holds the host twins below to it
 * and it to the truth, tests/test_gpu_deep_wide_bla.py holds the GPU to it, bit for bit).  Everything of "Extended-range deep
 * views" stands: the wide table, the offsets dcm 2^exp2, sh, norm, EZ, the steps (a) .. (g), counts, bytes, smooth, statistics
 * (pixel_iterations counts the reference's iterations -- count, or mrd - 1 for 0 -- not the steps executed).  Binary64
 * mantissas, int32 exponents, every floating operation rounded on its own, no contraction.
 *   numbers   a wide complex is (f_r, f_i, e) as norm produces it: the larger |component| in [0.5, 1), a zero is (0, 0, EZ).
 *             A wide real >= 0 is (f, e) with f in [0.5, 1), or (0, EZ): real(v, e) = (ldexp(v, -s), e + s) with s the frexp
 *             exponent of v > 0, (0, EZ) for v <= 0.  |(f_r, f_i, e)| = real(fl(sqrt(fl(fl(f_r^2) + fl(f_i^2)))), e).
 *             Wide reals compare by exponent, then by mantissa.  Complex products are the four-product form of the plain
 *             contract on the mantissas, (fl(fl(ac) - fl(bd)), fl(fl(ad) + fl(bc))) with (a, b) the left factor, at the sum of the
 *             exponents, not renormalised before the next operation (nominal exponents, as in the wide step).
 *   per view  dcmax = real(fl(|dcm_r(column 0)| + |dcm_i(row 0)|), exp2) of the FULL view, not the window (windows and bands
 *             share one table and stay bit-identical to the whole view; a render's sample view at s times the width and height
 *             is a full view of its own, as for MBK_DEEP_BLA).  eps = 2^-40.
 *   table     Level l has n_l = floor((M - 1) / 2^l) entries, for l = 0 .. while n_l >= 1 (at most 32 levels); entry j covers
 *             the 2^l steps that start at m = 1 + j 2^l.  With M <= 1 there is no table and the flag changes nothing.
 *             Level 0: A = (X_r, X_i, xe + 1) of the wide table's entry m (2 Z_m, exact; not renormalised, so a mantissa of
 *             exactly 1 stays), B = norm((1, 0), 0) = (0.5, 0, 1), r = (f, e - 40) with (f, e) = |A|.
 *             Level l + 1, entry j, from x = entry 2j and y = entry 2j + 1 of level l:
 *               A = norm(A_y A_x, e_Ay + e_Ax)
 *               B: Q = A_y B_x at qe = e_Ay + e_Bx;  h = max(qe, e_By);  B = norm(fl(sh(Q, qe - h) + sh(B_y, e_By - h)), h)
 *               t: (fa, ea) = |A_x|, (fb, eb) = |B_x|;  u = fl(fb f_dcmax) at ue = eb + e_dcmax;  g = max(e_ry, ue);
 *                  d = fl(sh(f_ry, e_ry - g) - sh(u, ue - g));  t = real(fl(d / fa), g - ea)
 *               r = min(r_x, t)
 *   dead      An entry is dead -- r = (0, EZ), A = B = (0, 0, EZ) stored -- when any of these holds: it is a level-0 entry with
 *             Z_m = 0; either child is dead; |A_x| = 0; d <= 0 (the radius max(t, 0) is 0); an exponent of the merged A or B
 *             other than EZ exceeds 2^20 in magnitude; the exponent of r is below -2^20.  A radius that small admits no dz a
 *             view with exp2 >= -8192 can hold; the bound keeps every sum of exponents inside int32 and EZ = -2^24 below every
 *             live exponent.  A dead entry is never taken and death propagates upward: this replaces the plain contract's
 *             "overflowed entries are never taken", and levels that overflow binary64 there are live here.
 *   radius    Per entry one int32 ke: the largest integer with 2^ke <= fl(f_r 0.7071067811865476) 2^e_r, that is
 *             e_r + (frexp exponent of that product) - 1; EZ for a dead entry.  A pixel state (w, q) passes iff EZ < q <= ke.
 *             max(|w_r|, |w_i|) < 1, so q <= ke puts both components of dz below 2^ke <= r / sqrt 2: one integer compare and one
 *             4-byte load per level probed, at the cost of at most a factor 2 in radius.  ke is non-increasing in l at a fixed
 *             starting m.  A zero dz (q = EZ) passes no entry: it takes the plain step, which keeps it at dc.
 *   step      state (w, q, m, i), i the index of the step about to run.  Take the highest level l with ALL of
 *               m >= 1;  (m - 1) mod 2^l = 0;  (m - 1) >> l < n_l;  i + 2^l <= mrd;  EZ < q <= ke
 *             (each is monotone in l: a search upward from level 0 that stops at the first failure finds the same level).
 *             If there is one:
 *               p1 = A w at e1 = e_A + q;  p2 = B dcm at e2 = e_B + exp2;  h = max(e1, e2)
 *               (w, q) = norm(fl(sh(p1, e1 - h) + sh(p2, e2 - h)), h);  m += 2^l
 *             and the step index becomes i + 2^l - 1.  If there is none, the steps (a) .. (d) run.  After either, (e), (f), (g)
 *             run exactly as in "Extended-range deep views", m == M included.  The steps inside a skip are not tested.
 *             m = 0, the state right after a rebase, always takes the plain step.  A zero dcm (the centre pixel of an odd-sized
 *             view) keeps its nominal exponent e_B + exp2, as in step (c); a zero B has e_B = EZ and never sets h.
 *   eps       2^-40, the plain contract's, held to the truth again here: against direct iteration at P + 128 bits the model
 *             equals the truth on every sampled pixel of the five cases of tests/test_deep_wide.py (spans 2^-1100 and 2^-3000
 *             on c = i and on a Misiurewicz point, and the centre 1e-400).  The cap is the wide contract's: >= 99 % of pixels.
 *
 * The ctx keeps the device copies of up to two such tables beside each orbit copy's wide table, keyed by the orbit's id and
 * dcmax (the bits of its mantissa and its exponent, which carries exp2): 4 + 48 bytes per entry, fewer than 2 (M - 1) entries
 * each.  They follow the rule of the MBK_DEEP_BLA tables: a table is built on the host and uploaded, synchronously, by the first
 * MBK_DEEP_XBLA launch on the ctx that brings its dcmax (the second place is allocated only then); once both places are taken
 * it goes over the table asked for least recently, and that first synchronises the device, since a queued launch may still
 * read the table it replaces.  Launch once per (orbit, spans) before capturing, and expect three or more dcmax in turn on one
 * orbit to serialise.  The tables are freed with the orbit copies.
 */
#define MBK_DEEP_XBLA 0x10000u
/* Host twins for the CPU tests, compiled from the functions the builder and the kernel use: no ctx, no device.  `view` gives
 * dcmax and exp2 (its window is not used); MBK_ERR_INVALID for what mbk_deep_xview_launch refuses in a view.
 * _info: the number of levels (0 for M <= 1) and of entries over all levels.  _read: level `level` into seven arrays of
 * capacity n (MBK_ERR_INVALID below n_level, or for a level the table does not have).  _count_host: the pixel (col, row) of
 * the full view under the rule above -- its count, the mag of the escaping step (0 for count 0) and the number of steps
 * executed, a skip counting as one. */
int mbk_deep_xbla_info(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t *levels, uint64_t *entries);
int mbk_deep_xbla_read(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t level, double *A_r, double *A_i,
                       int32_t *a_e, double *B_r, double *B_i, int32_t *b_e, int32_t *ke, uint64_t n);
int mbk_deep_xbla_count_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                             int32_t *count, double *mag, uint64_t *steps_executed);

/*
 * Distance estimates for deep views.  NOT in the reference; additive (the ABI version stays 5): no existing call changes, and
 * the plain-view contract above keeps its rule (dmag = |d|^2 overflows once |d| passes 1e154 and de is then 0).  |dz/dc| at
 * escape is of the order of 1 / (distance to the set): a view 1e-200 wide has |d| ~ 1e200 on every escaped pixel.  So the
 * derivative is carried as d = D 2^e with an integer e per pixel, and the value is reported as a fraction of the view's span.
 *
 * Contract (tests/deep_distance_model.py restates it in numpy; tests/test_gpu_deep_distance.py holds the GPU to it).
 * Everything of "Deep-zoom views" stands: orbit table, offsets dc, the step, rebasing, the count.  Added per pixel, binary64,
 * every operation rounded on its own:
 *   state     zp = the pixel's full z of the previous step, (Dr, Di) and an integer e with d = D 2^e.
 *             Start: zp = (fl(Z_1.r + dc.r), fl(Z_1.i + dc.i)) (z_0 = c), D = (1, 0), e = 0 -- the plain contract's d_0 = 1.
 *   step i    before the z step of the deep contract:
 *               u = fl(fl(zp.r Dr) - fl(zp.i Di)), v = fl(fl(zp.r Di) + fl(zp.i Dr)), Dr = fl(2u + one), Di = 2v,
 *               one = ldexp(1, -e) as a binary64 (subnormal, then 0, once e passes 1022);
 *             then, if max(|Dr|, |Di|) >= 2^256: Dr = fl(Dr 2^-256), Di = fl(Di 2^-256) (exact unless the smaller component
 *             turns subnormal), e = min(e + 256, 2^30).  Tested on EVERY step.  e never decreases; the cap only keeps the
 *             integer from wrapping (rel is 0 from e ~ 2200 on, with or without it).
 *             Then the deep step unchanged; zp becomes the z = fl(Z_m + dz) that step computes for its bailout test (after a
 *             rebase dz = z, so zp is the same value either way).  |D| < 2^256 and |zp| < 2^16.5: nothing overflows.
 *   count     n is exactly the count of mbk_deep_view_launch.
 *   run-on    a pixel with n > 0 first applies the deep step's rebase rule to the escaping step's state (mag < |dz|^2 or
 *             m == M: dz = z, m = 0 -- the count loop stops before it), then goes on, uncounted, with the same two recurrences
 *             (rebasing included, m == M included: m < M at the top of every step) until mag >= 2^32 or 64 further steps have
 *             run, as for plain views and for the reason given there.  mag is then at most ~2^64.
 *   output    the distance as a FRACTION OF THE VIEW'S REAL SPAN, rel = de / range_r, not a length in the plane (a length at
 *             span 2^-960 is near the bottom of binary64, and a render's scale, <= 2^80 per unit, could not reach it).  With
 *             range_r = f 2^k, 0.5 <= f < 1 (frexp), and dmagD = fl(fl(Dr^2) + fl(Di^2)) (below 2^513: no overflow),
 *               rel = ldexp(fl(fl(fl(sqrt(fl(mag / dmagD))) fl(ln mag)) / f), -(e + k)),
 *             ldexp rounding once where the result is subnormal.  0 if n = 0; never NaN (0 instead); dmagD = 0 gives +inf.
 *             ln is the device's (ocml), division and square root the correctly rounded ones.  The unit is the same for every
 *             window of a view and for every supersampling factor of a render (the sample view has the same range_r).
 *   mrd       0 and 1 run no step: every count and value is 0.
 * Windows of a view are bit-identical to the whole view.
 * Known limit: centres within ~1e-16 of -2 stay wrong, as their counts are ("Deep-zoom views", above).
 *
 * One pass: the derivative rides in the deep loop (csrc/mbk_deep_distance.h).  _launch_distance: DEVICE pointers on the caller's
 * stream (window-sized buffers, nothing is written outside them; no statistics).  _compute_distance: synchronous into HOST
 * buffers on slot 0 (the slot-0 rule applies), stats as for mbk_deep_view_compute (the run-on steps are not counted).
 * d_counts / h_counts may be NULL.  MBK_ERR_INVALID, with nothing written: a NULL d_rel / h_rel, any flag (there is no kernel
 * selection, no fp32, no MBK_LAZY_UNIFORM; MBK_WANT_* are not used either: the pointers select the outputs), and whatever
 * mbk_deep_view_launch refuses (NULL orbit, empty or oversized window, ranges outside [2^-960, 4], mrd > the orbit's mrd).
 */
int mbk_deep_view_launch_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                  uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream);
int mbk_deep_view_compute_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                   uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats);
/* "output" above on the HOST, compiled from the function the kernel uses (with the host's ln): no ctx, no device.  For the
 * CPU tests. */
double mbk_deep_distance_value_host(double mag, double dmagD, int32_t e, double range_r, int32_t count);

/*
 * Locating minibrots in deep views: atom periods, Newton seeds, refinement.  NOT in the reference; additive (the ABI version
 * stays 5): no existing call changes.  A deep view needs its centre as a decimal string of hundreds of digits; these calls
 * find such centres.  Per pixel the atom period -- the n at which |z_n| is smallest -- and one Newton step from the pixel
 * towards the root of z_p(c) = 0 come out of the loop that already carries the derivative; the refinement at full precision
 * and the size of the component found are host functions over a reference orbit and its wide table.
 *
 * Index convention.  The pixel's orbit is z_0 = c, z_{i+1} = z_i^2 + c with d_0 = 1, d_{i+1} = 2 z_i d_i + 1 (d_i = dz_i/dc),
 * as everywhere in the deep contracts; the reference table is Z_0 = 0, Z_1 = C, Z_{k+1} = Z_k^2 + C, so z_i corresponds to
 * Z_{i+1}.  A nucleus of period p has Z_p = 0, i.e. z_{p-1} = 0: the step arg at which |z_i| is smallest gives the
 * CONVENTIONAL period p = arg + 1, and that is what is stored.  On the table D_1 = 1, D_{k+1} = 2 Z_k D_k + 1 (D_k = dZ_k/dC).
 *
 * Contract of the device calls (tests/deep_nucleus_model.py restates it in numpy; tests/test_deep_nucleus.py holds the host
 * twin to it and it to the truth, tests/test_gpu_deep_nucleus.py holds the GPU to the host twin).  Everything of "Deep-zoom
 * views" stands (orbit table, offsets dc, the step, rebasing, the count) and so does the state and "step i" of "Distance
 * estimates for deep views" (zp, D, e, one, the 2^256 rescale on every step).  There is no run-on.  Added per pixel, binary64,
 * every operation rounded on its own:
 *   start     best = fl(fl(z_0.r^2) + fl(z_0.i^2)) (as mag is formed), arg = 0, kept state (z_b, D_b, e_b) = (z_0, (1, 0), 0).
 *   step i    (i = 1 .. mrd - 1) the derivative step, the z step, mag = |z_i|^2.  mag >= 4: n = i and the pixel ends; the
 *             escaping z is never a candidate.  Otherwise, if mag < best (strict: the first minimum wins): best = mag, arg = i,
 *             z_b = zp (the z of this step), (D_b, e_b) = (D, e).  Then the rebase rule, unchanged.
 *   period    arg + 1 (int32).
 *   count     n is exactly the count of mbk_deep_view_launch.
 *   delta     the Newton step -z_b / (D_b 2^e_b) as a FRACTION OF range_r, two binary64 per pixel (re, im).  With
 *             range_r = f 2^k, 0.5 <= f < 1 (frexp):
 *               den = fl(fl(D_b.r^2) + fl(D_b.i^2))
 *               N   = (fl(fl(z_b.r D_b.r) + fl(z_b.i D_b.i)), fl(fl(z_b.i D_b.r) - fl(z_b.r D_b.i)))           z_b conj(D_b)
 *               delta = ldexp(-fl(fl(N / den) / f), -(e_b + k)) per component (division correctly rounded, ldexp rounding once
 *             where the result is subnormal).  If either component is not finite both are stored as +inf: "no seed".
 *             delta does NOT include the pixel's own offset: the target is pixel offset + delta range_r, and the caller adds
 *             the offset exactly.
 *   mrd       0 and 1 run no step: count 0, period 1, delta from the start state (-z_0 as a fraction of range_r).
 * Windows of a view are bit-identical to the whole view.  Plain deep views only (spans 4 down to 2^-960; a shallow view is a
 * deep view too): an extended-range view has calls of its own ("Locating minibrots in extended-range deep views", below).
 *
 * One pass (csrc/mbk_deep_nucleus.h).  _launch_nucleus: DEVICE pointers on the caller's stream (d_period: int32 per pixel of the
 * window, d_delta: 2 binary64 per pixel; nothing is written outside them; no statistics).  _compute_nucleus: synchronous into
 * HOST buffers on slot 0 (the slot-0 rule applies), stats as for mbk_deep_view_compute.  d_counts / h_counts may be NULL.
 * MBK_ERR_INVALID, with nothing written: a NULL period or delta, any flag -- MBK_DEEP_BLA with a message of its own: a skipped
 * run has no |z_n| to compare -- and whatever mbk_deep_view_launch refuses.
 */
int mbk_deep_view_launch_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                 uint32_t flags, int32_t *d_counts, int32_t *d_period, double *d_delta, void *hip_stream);
int mbk_deep_view_compute_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                  uint32_t flags, int32_t *h_counts, int32_t *h_period, double *h_delta, mbk_stats *stats);
/* Host twin for the CPU tests, compiled from the functions the kernel uses: no ctx, no device.  The pixel (col, row) of the
 * full view: its count, period, best, z_b[2], D_b[2], e_b and delta[2].  MBK_ERR_INVALID for what the launch refuses. */
int mbk_deep_nucleus_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                          int32_t *count, int32_t *period, double *best, double *z_b, double *D_b, int32_t *e_b, double *delta);
/* Host only (no ctx, no device), in the wide number system of "Extended-range deep views" -- binary64 mantissa pairs, the
 * larger |component| in [0.5, 1), with one int32 exponent; a zero is (0, 0, -2^24):
 *   _newton_host   the Newton step at the orbit's own centre C, -Z_p / D_p = (d_r, d_i) 2^d_e.  Z_p is the wide table's entry,
 *                  correctly rounded from the fixed-point value, so a tiny Z_p keeps 53 bits: Newton reaches the orbit's
 *                  precision.  D_k is carried by "step i" of "Distance estimates for extended-range deep views" (what
 *                  mbk_deep_xdistance_step_host runs) from D_1 = 1.
 *   _size_host     the size estimate 1 / (b l^2) = (s_r, s_i) 2^s_e of the component whose nucleus C is:
 *                  l = prod_{k=1}^{p-1} 2 Z_k, b = 1 + sum_{k=1}^{p-1} 1 / l_k over the partial products l_k.  Period 1 gives
 *                  exactly 1.  A Z_k = 0 below p (p is not the minimal period) gives non-finite mantissas.
 * MBK_ERR_INVALID: a NULL argument, period 0, an orbit shorter than `period` (it escaped, or its mrd is below the period). */
int mbk_deep_orbit_newton_host(const mbk_deep_orbit *orbit, uint32_t period, double *d_r, double *d_i, int32_t *d_e);
int mbk_deep_orbit_size_host(const mbk_deep_orbit *orbit, uint32_t period, double *s_r, double *s_i, int32_t *s_e);

/*
 * Distance estimates for deep views with bilinear approximation.  NOT in the reference; additive (the ABI version stays 5): no
 * existing call changes -- mbk_deep_view_launch_distance / _compute_distance and the MBK_RENDER_DISTANCE_REL source of
 * mbk_deep_view_render_* keep refusing MBK_DEEP_BLA, the capability lives behind the names below.  Below spans of ~1e-15 a
 * view is drawn by its distance estimate, and those are the views with the largest iteration counts: here the estimate takes
 * the skips the count launches take (scripts/deep_distance_bla_rate.py, profiles/deep_distance_bla/).
 *
 * No second table.  d is the derivative of the pixel's full z = Z_m + dz with respect to c, and the reference orbit does not
 * depend on dc: across a skip dz -> A dz + B dc the derivative follows d -> A d + B with the A and B the table already holds.
 * The neglected terms are of the order of the |dz| / |Z| that the radius test bounds by eps = 2^-40 per step.
 *
 * Contract (tests/deep_distance_bla_model.py restates it in numpy; tests/test_deep_distance_bla.py holds the host twins below
 * to it and it to the truth, tests/test_gpu_deep_distance_bla.py holds the GPU to it).  Everything of "Deep-zoom views with
 * bilinear approximation" stands: the table and its bits, dcmax of the FULL view, eps, the level rule, the step index, and the
 * count, which is exactly the count mbk_deep_view_compute stores with MBK_DEEP_BLA.  Everything of "Distance estimates for deep
 * views" stands for a step that takes no level: zp, (D, e), one = ldexp(1, -e), u, v, Dr = fl(2u + one), Di = 2v, the 2^256
 * rescale tested on that step; and so do the start state and the output expression (unit rel).  Binary64, every operation
 * rounded on its own, no contraction.  Added:
 *   skip      a step that takes level l applies, BEFORE the dz map (as the plain derivative step comes before the z step), to
 *             d = D 2^e and the entry's (A, B):
 *               ea = the frexp exponent of max(|A_r|, |A_i|) (0 for 0);  As = ldexp(A, -ea)     (exact: larger part in [0.5, 1))
 *               eb = the frexp exponent of max(|B_r|, |B_i|) (0 for 0);  Bs = ldexp(B, -eb)
 *               P  = (fl(fl(As_r D_r) - fl(As_i D_i)), fl(fl(As_r D_i) + fl(As_i D_r)))
 *               pe = e + ea;  h = max(pe, eb, 0)
 *               N  = fl(ldexp(P, max(pe - h, -1200)) + ldexp(Bs, max(eb - h, -1200)))            per component
 *               then, if max(|N_r|, |N_i|) >= 2^256: N = fl(N 2^-256), h += 256 (once suffices: |N| < 2^258);
 *               else, if max(|N_r|, |N_i|) < 2^-256 and h >= 256: N = N 2^256 (exact), h -= 256;
 *               D = N, e = min(h, 2^30), one = ldexp(1, -e).
 *             The second rescale is what a long orbit needs: |As| < 1, so each skip may move up to a binade from D into e, and
 *             over the ~3000 skips of a pixel at mrd 30 000 D would decay (to 1e-207 on the seahorse view at 1e-20) until dmagD
 *             underflows and rel is +inf.  With it max(|D_r|, |D_i|) stays in [2^-256, 2^256) wherever e >= 256.
 *             It is finite for every entry that can be taken (A and B are finite binary64 up to 1e308, |D| < 2^256: the
 *             product is formed on mantissas).  An addend more than 1200 binades below the other is dropped, never wrapped.
 *             e stays a non-negative int32 at most 2^30, but it MAY DECREASE (|A| < 1 where the orbit passes near 0) and is no
 *             longer a multiple of 256: the "e never decreases" of "Distance estimates for deep views" is not part of this
 *             contract.  ea and eb are taken where the skip runs (frexp): nothing is stored beside the table, and what
 *             mbk_deep_bla_read returns does not change.
 *   rebase    after a skip zp becomes the z = fl(Z_m + dz) formed at the new m; D, e and zp do not change at a rebase.
 *   run-on    a pixel with n > 0 first applies the rebase rule to the escaping step's state, then runs PLAIN steps only --
 *             never a skip -- until mag >= 2^32 or 64 further steps have run.
 *   no skip   where no level is ever taken (M <= 1: no table; or a view whose offsets never pass the radius test) every state
 *             and rel equals "Distance estimates for deep views" bit for bit.
 *   mrd       0 and 1 run no step: every count and value is 0.
 * Windows of a view are bit-identical to the whole view.  Statistics: pixel_iterations counts the reference's iterations
 * (count, or mrd - 1 for 0), not the steps executed and not the run-on.
 * Against d' = 2 z d + 1, z' = z^2 + c in mpmath at P + 128 bits from the exact c, on the cases of tests/test_deep_distance.py:
 * (count, run-on) agree on >= 99 % of the escaped picks and rel is within DEEP_BLA_DERIVATIVE_REL of the model file.  The
 * error is NOT bounded by n 2^-39: it is a conditioning effect of the orbit-long product (measured figures in the model file).
 *
 * One pass (csrc/mbk_deep_distance_bla.h); with M <= 1 the launch is that of mbk_deep_view_launch_distance.  The argument rules
 * are those of the calls without _bla: device pointers on the caller's stream / host buffers synchronously on slot 0 with the
 * statistics above; counts may be NULL.  MBK_ERR_INVALID, with nothing written: a NULL rel, any flag -- MBK_DEEP_BLA too, with a
 * message of its own: the name selects the rule --, an orbit longer than 2^31 and whatever mbk_deep_view_launch refuses (mrd
 * above the orbit's, an empty window, ranges outside [2^-960, 4]).  The render calls take MBK_RENDER_DISTANCE_REL only: the
 * banding, supersampling and colour code of "Rendering" on these samples, as mbk_deep_xview_distance_render_* are for
 * extended-range views.  The ctx's tables are those of the MBK_DEEP_BLA count launches, keyed by the orbit's id and dcmax and
 * shared with them: launch once per (orbit, spans) before capturing, and expect three or more spans in turn on one orbit to
 * serialise.
 */
int mbk_deep_view_launch_distance_bla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                      uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream);
int mbk_deep_view_compute_distance_bla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                       uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats);
/* (mbk_deep_view_distance_bla_render_launch / _compute are declared under "Rendering", below.) */
/* Host twins for the CPU tests, compiled from the functions the kernel uses: no ctx, no device.  The pixel (col, row) of the
 * full view: its count, the run-on steps taken, the final mag (0 for count 0), the final D 2^e, rel (with the host's ln) and
 * the number of steps executed in the count loop, a skip counting as one.  MBK_ERR_INVALID for what the launch refuses. */
int mbk_deep_distance_bla_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                               int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e, double *rel,
                               uint64_t *steps_executed);
/* "skip" above, once: (D_r, D_i, e) in and out. */
int mbk_deep_distance_bla_skip_host(double A_r, double A_i, double B_r, double B_i, double *D_r, double *D_i, int32_t *e);

/*
 * Distance estimates for extended-range deep views.  NOT in the reference; additive (the ABI version stays 5): no existing
 * call changes -- mbk_deep_xview_render_* keeps refusing the distance sources, the capability lives behind the names below.
 * The views that need the estimate most are the deepest: at a span of 2^-1100 every visible structure is a filament thinner
 * than a sample.  The contract above cannot be stretched to them: its zp and its orbit table are binary64 and its spans stop
 * at 2^-960.  Here the derivative lives in the wide number system.
 *
 * Contract (tests/deep_wide_distance_model.py restates it in numpy; tests/test_deep_wide_distance.py holds the host twins
 * below to it and it to the truth, tests/test_gpu_deep_wide_distance.py holds the GPU to it).  Everything of "Extended-range
 * deep views" stands: the wide table, dcm 2^exp2, sh, norm, EZ, steps (a) .. (g), the counts.  Added per pixel, binary64
 * mantissas, int32 exponents, every operation rounded on its own, no contraction:
 *   state     zp = (zv_r, zv_i, t), the pixel's full z of the previous step: exactly the (zv, t) step (e) computes, kept wide
 *             and NOT renormalised (nominal exponent, as the wide step does).  D = (D_r, D_i, e), a wide complex as norm makes
 *             it, d = D 2^e.  Start: zp is step (e) applied to the entry 1 and the start state norm(dcm, exp2) (z_0 = c, taken
 *             before the M == 1 rebase, which leaves the same value); D = norm((1, 0), 0) = (0.5, 0, 1).
 *   step i    before the z step:
 *               P = (fl(fl(zv_r D_r) - fl(zv_i D_i)), fl(fl(zv_r D_i) + fl(zv_i D_r)))
 *               pe = t + e + 1 (the doubling is done in the exponent: exact);  h = max(pe, 0)
 *               N = (fl(sh(P_r, pe - h) + sh(1, -h)), sh(P_i, pe - h));  (D, e) = norm(N, h), then e = min(e, 2^30)
 *             Then steps (a) .. (g) unchanged; zp becomes the new (zv, t) (after a rebase dz = z: the same value either way).
 *   why wide  near a deep minibrot the orbit returns to within 1e-400 of 0 while |d| is 1e+400: a binary64 zp is 0 there and
 *             the product is lost.  For the same reason e may decrease.
 *   corners   sh clamps at -1200: with pe > ~1074 the +1 is dropped (it is below half an ulp unless P cancels); with
 *             pe < -1200 P is dropped and D = 1.  A zero D is (0, 0, EZ) and gives dmagD = 0, so rel = +inf, as in the plain
 *             rule.
 *   count     n is exactly the count of mbk_deep_xview_launch.
 *   run-on    as in "Distance estimates for deep views": a pixel with n > 0 first applies (g) to the escaping step's state, then
 *             runs the two recurrences uncounted (rebases and m == M included) until mag >= 2^32 or 64 further steps have run.
 *   output    rel = de / (range_r 2^exp2), the distance as a fraction of the view's real span.  With range_r = f 2^k (frexp)
 *             and dmagD = fl(fl(D_r^2) + fl(D_i^2)),
 *               rel = ldexp(fl(fl(fl(sqrt(fl(mag / dmagD))) fl(ln mag)) / f), -(e + k + exp2)),
 *             0 if n = 0; never NaN (0 instead).  The unit is the same for every window and every supersampling factor.
 *   equals plain  wherever a plain view can name the spans and no value of the plain run is subnormal, D 2^e is the plain
 *             contract's number (scaling by a power of two is exact) and rel is equal bit for bit.
 *   mrd       0 and 1 run no step: every count and value is 0.
 * Windows of a view are bit-identical to the whole view.
 * Against d' = 2 z d + 1, z' = z^2 + c in mpmath at P + 128 bits from the exact c: the (count, run-on) of every escaped pick
 * of the five truth cases of tests/test_deep_wide.py agree and rel is within WIDE_DERIVATIVE_REL of the model file.
 *
 * One pass (csrc/mbk_deep_wide_distance.h).  The two calls follow the rules of mbk_deep_view_launch_distance /
 * _compute_distance: device pointers on the caller's stream / host buffers synchronously on slot 0 with the statistics of
 * mbk_deep_xview_compute (the run-on steps are not counted); counts may be NULL.  MBK_ERR_INVALID, with nothing written: a
 * NULL rel, any flag (MBK_DEEP_XBLA and MBK_DEEP_BLA each with a message of its own: the derivative of a skipped run needs
 * coefficients of its own -- since built, behind names of its own: the next section) and whatever mbk_deep_xview_launch
 * refuses.
 */
int mbk_deep_xview_launch_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                   uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream);
int mbk_deep_xview_compute_distance(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                    uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats);
/* Host twins for the CPU tests, compiled from the functions the kernel uses: no ctx, no device.  The pixel (col, row) of the
 * full view: its count, the run-on steps taken, the final mag (0 for count 0), the final D 2^e and rel (with the host's ln).
 * MBK_ERR_INVALID for what the launch refuses. */
int mbk_deep_xview_distance_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                                 int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e, double *rel);
/* "step i" above, once: zp = (z_r, z_i) 2^t, (D_r, D_i, e) in and out. */
int mbk_deep_xdistance_step_host(double z_r, double z_i, int32_t t, double *D_r, double *D_i, int32_t *e);
/* "output" above. */
double mbk_deep_xdistance_value_host(double mag, double dmagD, int32_t e, double range_r, int32_t exp2, int32_t count);

/*
 * Locating minibrots in extended-range deep views.  NOT in the reference; additive (the ABI version stays 5): no existing call
 * changes -- mbk_deep_view_launch_nucleus / _compute_nucleus and mbk_deep_nucleus_host keep taking plain deep views only, the
 * capability lives behind the names below.  The minibrot found in a view of span s has a size of about s^2, so the view that
 * frames a nucleus located from a span of 1e-200 is 1e-401 wide: without these calls the chain view -> nucleus -> view stops
 * after one link, at the views whose centres have 400 to 1200 digits.  The index convention, the host refinement
 * (mbk_deep_orbit_newton_host / _size_host) and the meaning of period and delta are those of "Locating minibrots in deep
 * views".
 *
 * Contract (tests/deep_wide_nucleus_model.py restates it in numpy; tests/test_deep_wide_nucleus.py holds the host twin to it
 * and it to the truth, tests/test_gpu_deep_wide_nucleus.py holds the GPU to the host twin).  Everything of "Extended-range deep
 * views" stands: the wide table, dcm 2^exp2, sh, norm, EZ, steps (a) .. (g), rebasing with m == M included, the count.  So do
 * the state (zp, D, e), its start and "step i" of "Distance estimates for extended-range deep views": D = norm((1, 0), 0) =
 * (0.5, 0, 1), the derivative step before the z step.  There is no run-on.  Added per pixel, binary64 mantissas, int32
 * exponents, every operation rounded on its own, no contraction:
 *   nmag      the magnitude that orders the candidates is WIDE: near a deep minibrot |z| is 1e-400, |z|^2 as a binary64 (step
 *             (e)'s mag) is 0 and cannot order anything.  From the mg and t step (e) leaves, |z|^2 = mg 2^(2t), mg not
 *             normalised:  nmag(mg, t) = (bm, be) with s = the frexp exponent of mg, bm = ldexp(mg, -s) in [0.5, 1) (exact) and
 *             be = 2t + s;  mg == 0 gives (0, -2^30).  (bm', be') < (bm, be) iff be' < be, or be' == be and bm' < bm.
 *   start     best = nmag of z_0's (mg, t), arg = 0, kept state z_b = (zv_r, zv_i, t) exactly as step (e) left it (nominal
 *             exponent, NOT renormalised), (D_b, e_b) = (0.5, 0, 1).
 *   step i    (i = 1 .. mrd - 1) the derivative step, steps (a) .. (e), mag.  mag >= 4: n = i and the pixel ends; the escaping
 *             z is never a candidate.  Otherwise, if nmag(mg, t) < best (strict: the first minimum wins): best, arg = i,
 *             z_b = (zv, t) of this step and (D_b, e_b) = (D, e) are replaced.  Then (g), unchanged.
 *   period    arg + 1 (int32).
 *   count     n is exactly the count of mbk_deep_xview_launch.
 *   delta     the Newton step -z_b / (D_b 2^e_b) as a FRACTION OF THE VIEW'S REAL SPAN range_r 2^exp2, two binary64 per pixel
 *             (re, im).  With range_r = f 2^k, 0.5 <= f < 1 (frexp), on the mantissas:
 *               den = fl(fl(D_b.r^2) + fl(D_b.i^2))
 *               N   = (fl(fl(z_b.r D_b.r) + fl(z_b.i D_b.i)), fl(fl(z_b.i D_b.r) - fl(z_b.r D_b.i)))           z_b conj(D_b)
 *               delta = ldexp(-fl(fl(N / den) / f), t_b - e_b - k - exp2) per component (division correctly rounded, ldexp
 *             rounding once where the result is subnormal; underflow to 0 is a valid value).  If either component is not finite
 *             both are stored as +inf: "no seed".  delta does NOT include the pixel's own offset: the target is pixel offset +
 *             delta range_r, in units of 2^exp2, and the caller adds the offset exactly.
 *   equals plain  the kept states of this contract and of the plain one differ by exact powers of two only, so wherever a plain
 *             view can name the spans and no value of the plain run is subnormal, period, count and delta are the plain
 *             contract's, bit for bit.
 *   mrd       0 and 1 run no step: count 0, period 1, delta from the start state.
 * Windows of a view are bit-identical to the whole view.
 *
 * One pass (csrc/mbk_deep_wide_nucleus.h).  The two calls follow the rules of mbk_deep_view_launch_nucleus / _compute_nucleus:
 * device pointers on the caller's stream (d_period: int32 per pixel of the window, d_delta: 2 binary64 per pixel; nothing is
 * written outside them; no statistics) / host buffers synchronously on slot 0 with the statistics of mbk_deep_xview_compute;
 * counts may be NULL.  MBK_ERR_INVALID, with nothing written: a NULL period or delta, any flag -- MBK_DEEP_XBLA and
 * MBK_DEEP_BLA each with a message of its own: a skipped run has no |z_n| to compare -- and whatever mbk_deep_xview_launch
 * refuses.
 */
int mbk_deep_xview_launch_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                  uint32_t flags, int32_t *d_counts, int32_t *d_period, double *d_delta, void *hip_stream);
int mbk_deep_xview_compute_nucleus(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                   uint32_t flags, int32_t *h_counts, int32_t *h_period, double *h_delta, mbk_stats *stats);
/* Host twin for the CPU tests, compiled from the functions the kernel uses: no ctx, no device.  The pixel (col, row) of the
 * full view: its count, period, best = (best_m, best_e), z_b[2] with t_b, D_b[2] with e_b and delta[2].  MBK_ERR_INVALID for
 * what the launch refuses. */
int mbk_deep_xview_nucleus_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                                int32_t *count, int32_t *period, double *best_m, int32_t *best_e, double *z_b, int32_t *t_b, double *D_b,
                                int32_t *e_b, double *delta);

/*
 * Distance estimates for extended-range deep views with bilinear approximation.  NOT in the reference; additive (the ABI
 * version stays 5): no existing call changes -- mbk_deep_xview_launch_distance / _compute_distance and the renders on them keep
 * refusing MBK_DEEP_XBLA, the capability lives behind the names below, as *_distance_bla does for plain deep views.  Below
 * spans of 2^-960 the distance picture is the one a user wants and the step is the most expensive of the library; this was
 * the last deep output that ran every step.  No second table: d is the derivative of the pixel's full z = Z_m + dz and the
 * reference orbit does not depend on dc, so across a skip dz -> A dz + B dc the derivative follows d -> A d + B with the A and
 * B the table of "Extended-range deep views with bilinear approximation" already holds.
 *
 * Contract (tests/deep_wide_distance_bla_model.py restates it in numpy; tests/test_deep_wide_distance_bla.py holds the host
 * twins below to it and it to the truth, tests/test_gpu_deep_wide_distance_bla.py holds the GPU to it).  Everything of
 * "Extended-range deep views with bilinear approximation" stands: the table and its bits, dcmax of the FULL view, eps = 2^-40,
 * ke and the level rule, the step index, the apply rule (p1, p2, h, norm), the tail (e), (f), (g), and the count, which is
 * exactly the count mbk_deep_xview_compute stores with MBK_DEEP_XBLA.  Everything of "Distance estimates for extended-range
 * deep views" stands for a step that takes no level: zp = (zv, t), D = (D_r, D_i, e) as norm makes it, step i, the start state
 * (0.5, 0, 1), the output expression and its unit rel.  Binary64 mantissas, int32 exponents, every operation rounded on its
 * own, no contraction.  Added:
 *   skip      a step that takes level l applies, BEFORE the dz map (as the plain derivative step comes before the z step), to
 *             d = D 2^e and the entry's (A, e_A), (B, e_B):
 *               P  = (fl(fl(A_r D_r) - fl(A_i D_i)), fl(fl(A_r D_i) + fl(A_i D_r))),  pe = e_A + e
 *               h  = max(pe, e_B)
 *               N  = fl(sh(P, pe - h) + sh(B, e_B - h))                                       per component
 *               (D, e) = norm(N, h), then e = min(e, 2^30)
 *             No 2^256 rescale and no floor at 0: norm does both jobs.  A zero D has exponent EZ and never sets h (a live A
 *             is non-zero, |e_A| <= 2^20).  An addend more than 1200 binades below the other is dropped by sh, never wrapped.
 *             e may decrease (|A| < 1 where the orbit passes near 0).  Nothing is stored beside the table, and what
 *             mbk_deep_xbla_read returns does not change.
 *   zp        after a skip zp becomes the (zv, t) that step (e) forms at the new m; D, e and zp do not change at a rebase.
 *   run-on    a pixel with n > 0 first applies (g) to the escaping step's state, then runs PLAIN steps only -- never a skip --
 *             until mag >= 2^32 or 64 further steps have run.
 *   no skip   where no level is ever taken (M <= 1: no table; or a view such as the centre 1e-400 at span 4, whose level 0 is
 *             never within its radius) every state and rel equals mbk_deep_xview_launch_distance bit for bit.
 *   mrd       0 and 1 run no step: every count and value is 0.
 * Windows of a view are bit-identical to the whole view.  Statistics: pixel_iterations counts the reference's iterations
 * (count, or mrd - 1 for 0), not the steps executed and not the run-on.
 * Against d' = 2 z d + 1, z' = z^2 + c in mpmath at P + 128 bits from the exact c, on the five truth cases of
 * tests/test_deep_wide.py: (count, run-on) agree on >= 99 % of the escaped picks and rel is within XBLA_DERIVATIVE_REL of the
 * model file, which holds the measured figures.  What a skip neglects is of the order of the |dz| / |Z| that the radius test
 * bounds by 2^-40 per step; the error of rel is that times the conditioning of the orbit-long product.
 *
 * One pass (csrc/mbk_deep_wide_distance_bla.h); with M <= 1 the launch is that of mbk_deep_xview_launch_distance.  The argument
 * rules are those of the calls without _xbla: device pointers on the caller's stream / host buffers synchronously on slot 0
 * with the statistics above; counts may be NULL.  MBK_ERR_INVALID, with nothing written: a NULL rel, any flag -- MBK_DEEP_XBLA
 * and MBK_DEEP_BLA each with a message of its own: the name selects the rule --, an orbit longer than 2^31 and whatever
 * mbk_deep_xview_launch refuses.  The render calls take MBK_RENDER_DISTANCE_REL only: banding, supersampling, colour,
 * statistics and refusals are those of mbk_deep_xview_distance_render_*; the sample view at s x is a full view of its own and
 * has a table of its own, as for MBK_DEEP_XBLA.  The ctx's tables are those of the MBK_DEEP_XBLA count launches, keyed by the
 * orbit's id and dcmax and shared with them: launch once per (orbit, spans) before capturing, and expect three or more spans
 * in turn on one orbit to serialise.
 */
int mbk_deep_xview_launch_distance_xbla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                        uint32_t flags, int32_t *d_counts, double *d_rel, void *hip_stream);
int mbk_deep_xview_compute_distance_xbla(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                         uint32_t flags, int32_t *h_counts, double *h_rel, mbk_stats *stats);
/* (mbk_deep_xview_distance_xbla_render_launch / _compute are declared under "Rendering", below.) */
/* Host twins for the CPU tests, compiled from the functions the kernel uses: no ctx, no device.  The pixel (col, row) of the
 * full view: its count, the run-on steps taken, the final mag (0 for count 0), the final D 2^e, rel (with the host's ln) and
 * the number of steps executed in the count loop, a skip counting as one.  MBK_ERR_INVALID for what the launch refuses. */
int mbk_deep_xview_distance_xbla_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row, uint32_t mrd,
                                      int32_t *count, int32_t *extra, double *mag, double *D_r, double *D_i, int32_t *e, double *rel,
                                      uint64_t *steps_executed);
/* "skip" above, once: A = (A_r, A_i) 2^a_e, B = (B_r, B_i) 2^b_e, (D_r, D_i, e) in and out. */
int mbk_deep_xdistance_skip_host(double A_r, double A_i, int32_t a_e, double B_r, double B_i, int32_t b_e, double *D_r, double *D_i,
                                 int32_t *e);

/*
 * Rendering: a view to an RGBA8 image on the device, with a palette and supersampling.  Replaces, for a view of any kind,
 * what the reference's Viewer does on the host for a chunk (DistributedMandelbrotViewer.py:110-135, data_to_img_array: the
 * bytes through matplotlib's jet, black where the byte is 0) -- mbk_palette_viewer is that colouring as a palette.  Additive
 * (the ABI version stays 5): no existing call changes.
 *
 * Contract (bit-exact given the samples; tests/render_model.py restates it in numpy, tests/test_gpu_render.py holds the GPU to
 * it).  A render of a view of W x H OUTPUT pixels with supersampling factor s:
 *   samples   the sample view covers the same rectangle (start_*, range_*; for a deep view the same orbit and range_*) with
 *             width W s and height H s.  Output pixel (x, y) owns sample columns x s .. x s + s - 1 and sample rows
 *             y s .. y s + s - 1, and an output window (col0, row0, ncols, nrows) is the sample window scaled by s.  The samples
 *             are exactly what mbk_view_launch (MBK_WANT_BYTES) / mbk_view_launch_smooth / mbk_deep_view_launch write for that
 *             sample view with the kernel the flags select.  With end points included the s times finer linspace is NOT centred
 *             on the pixels of the s = 1 view: a render with s > 1 is the box filter of the finer view, not of the same one.
 *   colour    of one sample, RGBA8, from the caller's palette p of n RGBA8 entries:
 *             MBK_RENDER_BYTES (n = 256): p[b], b the sample's quantised byte.
 *             MBK_RENDER_SMOOTH (2 <= n <= 65536): `inside` if the sample's count is 0 (decided on the count, not on nu).
 *             Otherwise, in binary64, every operation rounded on its own: t = fl(fl(nu * scale) + offset); t = 0 unless
 *             0 <= t (negative, -inf, NaN); k = floor(t), f = floor((t - k) * 256) (both exact), i0 = k mod n,
 *             i1 = (k + 1) mod n, and per channel (p[i0] (256 - f) + p[i1] f + 128) >> 8 in integers.  0 < scale <= 2^20 and
 *             |offset| <= 2^20, so t < 2^52 for every nu a launch can produce (nu < 2^31 + 1; a t >= 2^52, which only
 *             mbk_render_resolve_host can be handed, is taken as 0 too).
 *   resolve   per channel, alpha included, with S the sum over the pixel's s^2 sample colours: (2 S + s^2) / (2 s^2) rounded
 *             down (round half up; the identity for s = 1).  s is 1, 2, 3, 4 or 8.  The 8-bit palette values are averaged as
 *             they are: the palette is in whatever colour space the caller wants.
 *   output    uint8[nrows][ncols][4], row 0 the lowest imaginary part as everywhere else.
 *
 * Memory.  The samples never leave the device: they live in a scratch buffer the ctx keeps PER STREAM (like the launches'
 * other scratch), which grows on demand up to MBK_RENDER_BAND_BYTES and no further.  The output window is cut into bands of
 * rows -- and pieces of columns, should a single row's samples exceed the budget -- whose samples fit: 12 bytes per sample
 * (int32 count + binary64 nu) for MBK_RENDER_SMOOTH, 1 byte for MBK_RENDER_BYTES through _launch and 5 through _compute (the
 * counts feed the statistics).  A 4096-wide render at s = 4 takes bands of 341 rows; a 4096 x 4096 smooth render at s = 1 is one
 * band of 192 MiB.  max_band_rows lowers the band height further.  Windows of a view are bit-identical to the whole view, so
 * banding cannot change the image.  Beside the samples a stream keeps its palette on the device (<= 256 KiB), and _compute
 * keeps one device image of 4 bytes per output pixel of the largest window rendered, per ctx.  The palette is copied during
 * the call; a call whose palette or palette length differs from the previous render's on that stream first waits for the
 * stream (like an orbit's first launch: render once before capturing renders into a graph -- "Graph capture": inside a capture
 * a render with another palette is refused).
 *
 * Out of scope: handing bands to several GPUs (sharding.py; a band of an image is a window, and windows are bit-identical,
 * so a follow-up can), slot / submit forms, gamma-aware averaging, and fusing the colouring into the escape kernels.
 * (Decoding stored chunk streams on the device: "Stored chunks", below.)
 */
#define MBK_RENDER_BYTES 0u
#define MBK_RENDER_SMOOTH 1u
/* MBK_RENDER_DISTANCE (plain views only; a deep render refuses it and takes MBK_RENDER_DISTANCE_REL): the samples are what mbk_view_launch_distance writes for
 * the sample view (12 bytes per sample, banded like MBK_RENDER_SMOOTH).  Colour of a sample: `inside` if its count is 0;
 * otherwise the MBK_RENDER_SMOOTH rule with de in place of nu -- t = fl(fl(de * scale) + offset), t = 0 unless 0 <= t --
 * except that the palette does NOT wrap: t >= n - 1 (+inf included) gives p[n - 1], otherwise k = floor(t),
 * f = floor((t - k) * 256) and p[k], p[k + 1] are blended as above.  2 <= n <= 65536, |offset| <= 2^20 and, for this source
 * only, 0 < scale <= 2^80 (de of a view 1e-13 wide is ~1e-16: scale is in units of 1 / pitch).  mbk_render_resolve_host takes
 * the source too, reading de through its `smooth` argument.  mbk_julia_view_distance_render_* ("Distance estimates for Julia
 * views") takes this source and no other, on the samples of mbk_julia_view_launch_distance; mbk_julia_view_render_* refuses it. */
#define MBK_RENDER_DISTANCE 3u
/* MBK_RENDER_DISTANCE_REL (deep renders only; a plain render refuses it): the samples are what mbk_deep_view_launch_distance
 * writes for the sample view (12 bytes per sample, banded like MBK_RENDER_SMOOTH): rel, the distance as a fraction of the
 * view's real span, the same unit at every supersampling factor.  Colour: the MBK_RENDER_DISTANCE rule with rel in place of
 * de (no wrap, `inside` for count 0, 0 < scale <= 2^80): a ramp over w output pixels of a W-wide view has
 * scale = (n - 1)(W - 1) / w.  mbk_render_resolve_host takes the source too. */
#define MBK_RENDER_DISTANCE_REL 4u
/* MBK_RENDER_EQUALIZED (plain and deep views, through the mbk_*_render_equalized_* calls only: the four calls below have no
 * table and refuse it): the samples are those of MBK_RENDER_SMOOTH, coloured through an equalisation table -- "Count histograms
 * and histogram-equalised colouring", below. */
#define MBK_RENDER_EQUALIZED 5u
/* The most sample scratch a render keeps on one stream. */
#define MBK_RENDER_BAND_BYTES (256u << 20)

typedef struct mbk_render_spec {
    uint32_t source;        /* MBK_RENDER_BYTES | MBK_RENDER_SMOOTH | MBK_RENDER_DISTANCE | MBK_RENDER_DISTANCE_REL | MBK_RENDER_EQUALIZED */
    uint32_t supersample;   /* 1, 2, 3, 4, 8 */
    const uint8_t *palette; /* HOST pointer, palette_len x RGBA8; copied during the call */
    uint32_t palette_len;
    uint8_t inside[4];      /* MBK_RENDER_SMOOTH, _DISTANCE: the colour of a sample that never escapes */
    double scale, offset;   /* MBK_RENDER_SMOOTH, _DISTANCE; ignored (not validated) for MBK_RENDER_BYTES */
    uint32_t max_band_rows; /* 0 = the library's choice; any value gives the same image */
} mbk_render_spec;

/* Asynchronous, on the caller's stream: d_rgba is a DEVICE buffer of ncols * nrows * 4 bytes, and nothing is written outside
 * it.  `flags` carries kernel selection (and MBK_PRECISION_F32 for MBK_RENDER_BYTES) only, under the rules of the call that
 * makes the samples: MBK_RENDER_SMOOTH refuses MBK_KERNEL_SIMPLE / _REFILL / MBK_PRECISION_F32, a deep render refuses every
 * flag but MBK_DEEP_BLA.  MBK_ERR_INVALID, with nothing written: a NULL spec / palette / output, an unknown source, s outside the set,
 * palette_len wrong for the source, scale / offset outside their ranges or not finite, W s or H s beyond what the sample call
 * accepts (the whole sample window is validated as one), any other flag, and whatever the sample call refuses.
 * _compute: synchronous into a HOST buffer on slot 0 (the slot-0 rule above applies); stats as for mbk_view_compute, over the
 * SAMPLES: pixel_iterations, never_pixels; d2h_ms the copy of the image; all_bytes_* and rle_runs are 0; kernel_ms runs from
 * the first sample kernel to the last resolve kernel (with several bands it includes the statistics passes between them).
 * mbk_serialize_last still refers to the last tile computed with bytes: a render does not touch it. */
int mbk_view_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                           uint8_t *d_rgba, void *hip_stream);
int mbk_view_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                            uint8_t *h_rgba, mbk_stats *stats);
int mbk_deep_view_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
/* Extended-range deep views ("Extended-range deep views"): sources MBK_RENDER_BYTES / _SMOOTH (and _EQUALIZED through the
 * _equalized_ calls below); MBK_RENDER_DISTANCE, MBK_RENDER_DISTANCE_REL and every flag but MBK_DEEP_XBLA ("Extended-range
 * deep views with bilinear approximation": the samples are then those of mbk_deep_xview_launch with the flag) are
 * MBK_ERR_INVALID. */
int mbk_deep_xview_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                 uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_deep_xview_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                  uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_deep_view_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                 uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
/* Distance renders of extended-range deep views ("Distance estimates for extended-range deep views"), calls of their own as
 * the interior renders are: the source must be MBK_RENDER_DISTANCE_REL, the samples are what mbk_deep_xview_launch_distance
 * writes for the sample view, and colour, banding, supersampling, statistics and refusals are those of a deep render with
 * that source.  Every flag is MBK_ERR_INVALID. */
int mbk_deep_xview_distance_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_deep_xview_distance_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
/* Distance renders of deep views that take skips ("Distance estimates for deep views with bilinear approximation"), calls of
 * their own in the same way: the source must be MBK_RENDER_DISTANCE_REL, the samples are what mbk_deep_view_launch_distance_bla
 * writes for the sample view, and colour, banding, supersampling, statistics and refusals are those of a deep render with that
 * source.  Every flag is MBK_ERR_INVALID. */
int mbk_deep_view_distance_bla_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                             uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_deep_view_distance_bla_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                              uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
/* Distance renders of extended-range deep views that take skips ("Distance estimates for extended-range deep views with
 * bilinear approximation"), calls of their own in the same way: the source must be MBK_RENDER_DISTANCE_REL, the samples are
 * what mbk_deep_xview_launch_distance_xbla writes for the sample view, and colour, banding, supersampling, statistics and
 * refusals are those of mbk_deep_xview_distance_render_*.  Every flag is MBK_ERR_INVALID. */
int mbk_deep_xview_distance_xbla_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                               uint32_t flags, const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_deep_xview_distance_xbla_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                                uint32_t flags, const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
/* The reference Viewer's colouring as a 256-entry palette for MBK_RENDER_BYTES, host only: entry 0 black (0, 0, 0, 255),
 * entry b = jet(1 - b / 256) as data_to_img_array evaluates it, each channel floor(255 x + 0.5) (jet holds exact .5 ties, so
 * the rounding rule is part of the contract).  Computed from jet's public definition (its knots and matplotlib's 256-entry
 * table construction, every operation rounded on its own); held to the reference Viewer's recorded output, all 1024 bytes, by
 * tests/test_render.py (tests/golden/viewer_palette.npz). */
int mbk_palette_viewer(uint8_t out[1024]);
/* "Colour" and "resolve" above applied on the HOST to caller-supplied samples of (width s) x (height s), row-major: no ctx, no
 * device; the same functions the kernel is compiled from.  For the CPU tests.  MBK_RENDER_SMOOTH reads counts and smooth,
 * MBK_RENDER_BYTES reads bytes; the others may be NULL.  rgba: width * height * 4 bytes.  MBK_ERR_INVALID as above, and for
 * a width or height of 0 or width s, height s >= 2^31. */
int mbk_render_resolve_host(const mbk_render_spec *spec, uint32_t width, uint32_t height, const int32_t *counts,
                            const uint8_t *bytes, const double *smooth, uint8_t *rgba);

/*
 * Adaptive supersampling: the s x s samples of a render are computed only for the output pixels that straddle a colour edge.
 * NOT in the reference; additive (the ABI version stays 5): no existing call, flag or default changes.  Plain Mandelbrot views
 * (mbk_view) and MBK_RENDER_SMOOTH only.  A render at s = 8 computes 64 samples for every pixel; away from the boundary of the
 * set neighbouring pixels take nearly the same colour and the mean of 64 samples is what one sample gives.
 *
 * Contract (all integer arithmetic past the samples' colours; tests/adaptive_model.py restates it in numpy,
 * tests/test_adaptive.py holds the host twin and tests/test_gpu_adaptive.py the GPU to it).  Given a view of W x H output
 * pixels, a window of it, a factor s in {1, 2, 3, 4, 8}, an mbk_render_spec and a threshold in [0, 256]:
 *   base      B[y][x] is the colour mbk_view_render_launch gives pixel (x, y) at supersample = 1: the MBK_RENDER_SMOOTH colour
 *             of sample (x, y) of the W x H view, count and nu exactly as mbk_view_launch_smooth stores them.  It is defined
 *             over the whole view, not the window.
 *   N(x, y)   the up to eight pixels (x + dx, y + dy), dx, dy in {-1, 0, 1} and not both 0, that lie inside the FULL view:
 *             clamped at the view's edges, never at the window's or a band's.
 *   diff      diff(p, q) = the largest |p.ch - q.ch| over the four channels, alpha included.
 *   refined   pixel (x, y) is refined iff threshold == 0, or some q in N(x, y) has diff(B[y][x], B[q]) >= threshold.  So
 *             threshold 0 refines every pixel (a 1 x 1 view's too) and 256 none.
 *   output    a refined pixel is exactly the pixel of mbk_view_render_launch at factor s (the rounded mean of the colours of
 *             its s x s samples of the W s x H s view, "resolve" above); any other pixel is B[y][x].  Threshold 0 therefore
 *             gives the existing render at s bit for bit, threshold 256 the existing render at 1, and s = 1 the existing
 *             render at every threshold.  A window or a band is bit-identical to the same rectangle of the whole image.
 *   mask      optional, uint8[nrows][ncols]: 1 where refined, 0 elsewhere; of the window, decided on the full view.
 *   stats     (_compute) pixel_iterations and never_pixels count the base samples of the window's own pixels plus the s^2
 *             samples of each refined pixel of the window (at s = 1 that one sample is the base sample: counted once); the
 *             halo below is not counted and nothing is counted twice across bands.  The other fields are
 *             mbk_view_render_compute's.
 *
 * How it runs (csrc/mbk_adaptive.h).  Per band: the base samples of the band grown by one pixel on each side and clamped to the
 * view, by the sample kernels the flags select; a classify kernel that colours them, writes B, the mask and a list of the
 * refined pixels; a refine kernel that computes the s^2 samples of each listed pixel, one lane per sample.  The length of the
 * list stays on the device: the launch form is asynchronous on the caller's stream, waits for nothing but the palette's
 * change (as every render) and, once the same call has been made outside a capture, can be captured into a graph at every
 * size of band ("Graph capture" has the rules: the warm-up, what a capture changes in the base pass, how long a graph stays
 * valid).  Scratch: 12 bytes per base sample of the
 * haloed band plus 4 per pixel of the band for the list, within MBK_RENDER_BAND_BYTES; max_band_rows keeps its meaning.
 * _compute keeps one byte per pixel for the mask behind the ctx' device image.
 *
 * `flags` are those mbk_view_render_* accepts for MBK_RENDER_SMOOTH: kernel selection, which applies to the base pass;
 * MBK_KERNEL_ASM also runs the refine kernel on the per-step loop instead of the grouped loop with the cycle test (same
 * image).  MBK_ERR_INVALID, with nothing written: whatever mbk_view_render_* refuses for MBK_RENDER_SMOOTH, any other source,
 * threshold > 256, MBK_PRECISION_F32.  d_mask / h_mask may be NULL.
 *
 * Out of scope: Julia views (one more kind of sample launch on the same three steps; deep and extended-range deep views have
 * sections of their own below); the
 * bytes, distance and equalised sources; a distance-guided criterion, which would also catch filaments thinner than a pixel
 * inside a region of one colour (this criterion sees only what the s = 1 samples hit); sharding and slot forms.
 */
int mbk_view_render_adaptive_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                    uint32_t threshold, uint8_t *d_rgba, uint8_t *d_mask, void *hip_stream);
int mbk_view_render_adaptive_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_render_spec *spec,
                                     uint32_t threshold, uint8_t *h_rgba, uint8_t *h_mask, mbk_stats *stats);
/* The contract on the HOST for caller-supplied samples, no ctx, no device; compiled from the functions the kernels use.
 * base_*: the samples of the FULL width x height view; fine_*: those of the FULL (width s) x (height s) view, row-major.
 * rgba: width * height * 4 bytes; mask: width * height bytes or NULL.  MBK_ERR_INVALID as above, for a NULL sample array or
 * rgba, and for a width or height of 0 or width s, height s >= 2^31. */
int mbk_render_adaptive_host(const mbk_render_spec *spec, uint32_t threshold, uint32_t width, uint32_t height,
                             const int32_t *base_counts, const double *base_smooth, const int32_t *fine_counts,
                             const double *fine_smooth, uint8_t *rgba, uint8_t *mask);

/*
 * Adaptive supersampling of deep views: the same for mbk_deep_view, with the plain step and with MBK_DEEP_BLA.  NOT in the
 * reference; additive (the ABI version stays 5): no existing call, flag or default changes.  A deep sample costs thousands of
 * perturbation steps, and mbk_deep_view_render_* at factor s pays s^2 of them for every pixel.
 *
 * Contract: that of "Adaptive supersampling" word for word (tests/adaptive_model.py; tests/test_deep_adaptive.py and
 * tests/test_gpu_deep_adaptive.py hold the host twin and the GPU to it), with
 *   base      B[y][x] the MBK_RENDER_SMOOTH colour of sample (x, y) of the W x H view, count and nu exactly as
 *             mbk_deep_view_launch stores them;
 *   refined   pixel: the pixel of mbk_deep_view_render_launch at factor s;
 *   flags     0 or MBK_DEEP_BLA.  With the bit set both kinds of sample are those of MBK_DEEP_BLA: the base samples step with
 *             the table of the W x H view's dcmax, the fine samples with the table of the (W s) x (H s) view's -- the two
 *             differ for many shapes, since dcmax is formed from the half-widths in samples -- which is exactly what
 *             mbk_deep_view_render_* with the flag uses at 1 and at s.
 * So threshold 0 equals mbk_deep_view_render_* at s bit for bit, threshold 256 equals it at 1, s = 1 equals it at 1 at every
 * threshold, and a window or a band is bit-identical to the same rectangle of the whole image.  The mask and the stats keep
 * their meaning: the stats count the stored counts of the window's base samples plus the s^2 fine samples of each refined
 * pixel, the halo is not counted, and with MBK_DEEP_BLA they follow the counts, not the steps executed.
 *
 * How it runs (csrc/mbk_deep_adaptive.h).  The three steps, the scratch layout, the band plan, the halo, the palette staging and
 * _compute's mask placement are those above; the base pass is the deep sample launch and the refine kernel computes the listed
 * pixels' fine samples by perturbation, one lane per sample, with the table's skips under MBK_DEEP_BLA (an orbit of length 1
 * has no table: the flag changes nothing).  The ctx keeps TWO tables beside each orbit copy (see "Deep-zoom views with bilinear
 * approximation"); a render with the flag acquires the base view's and the fine view's together before it enqueues anything,
 * and neither takes the other's place (equal dcmax: one table).  A first call with a given (orbit, view, s) may therefore build
 * and upload synchronously; after it the launch form performs no host synchronisation for as long as both tables stay
 * resident -- until a launch on the same orbit brings a third dcmax -- and can be captured into a graph ("Graph capture": a
 * graph must not be replayed after that third dcmax either).
 *
 * MBK_ERR_INVALID, with nothing written: whatever mbk_deep_view_render_* refuses for MBK_RENDER_SMOOTH, any other source,
 * threshold > 256, any flag but MBK_DEEP_BLA (MBK_DEEP_XBLA with a message of its own).  d_mask / h_mask may be NULL.
 *
 * Out of scope: Julia views; the equalised, bytes and MBK_RENDER_DISTANCE_REL sources; a distance-guided criterion; sharding
 * and slot forms.  (mbk_deep_xview: the next section.)
 */
int mbk_deep_view_render_adaptive_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                         uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *d_rgba,
                                         uint8_t *d_mask, void *hip_stream);
int mbk_deep_view_render_adaptive_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *h_rgba,
                                          uint8_t *h_mask, mbk_stats *stats);

/*
 * Adaptive supersampling of extended-range deep views: the same for mbk_deep_xview, with the plain wide step and with
 * MBK_DEEP_XBLA.  NOT in the reference; additive (the ABI version stays 5): no existing call, flag or default changes.  A wide
 * sample is the most expensive in the library -- every step aligns with ldexp and renormalises with frexp, and the orbits are
 * the longest -- and mbk_deep_xview_render_* at factor s pays s^2 of them for every pixel.
 *
 * Contract: that of "Adaptive supersampling" word for word (tests/adaptive_model.py; tests/test_deep_wide_adaptive.py and
 * tests/test_gpu_deep_wide_adaptive.py hold the shares and the GPU to it), with
 *   base      B[y][x] the MBK_RENDER_SMOOTH colour of sample (x, y) of the W x H view, count and nu exactly as
 *             mbk_deep_xview_launch stores them, with MBK_DEEP_XBLA if set;
 *   refined   pixel: the pixel of mbk_deep_xview_render_launch at factor s;
 *   flags     0 or MBK_DEEP_XBLA.  With the bit set both kinds of sample are those of MBK_DEEP_XBLA: the base samples step with
 *             the table of the W x H view's dcmax, the fine samples with the table of the (W s) x (H s) view's -- 65 x 45 at
 *             exp2 -1100 differs from its fine view at every s, 67 x 45 at none -- which is exactly what
 *             mbk_deep_xview_render_* with the flag uses at 1 and at s.
 * So threshold 0 equals mbk_deep_xview_render_* at s bit for bit, threshold 256 equals it at 1, s = 1 equals it at 1 at every
 * threshold, and a window or a band is bit-identical to the same rectangle of the whole image.  The mask and the stats keep
 * their meaning: the stats count the stored counts of the window's base samples plus the s^2 fine samples of each refined
 * pixel, the halo is not counted, and with MBK_DEEP_XBLA they follow the counts, not the steps executed.
 *
 * How it runs (csrc/mbk_deep_wide_adaptive.h).  The three steps, the scratch layout, the band plan, the halo, the palette
 * staging and _compute's mask placement are those above; the base pass is the wide sample launch and the refine kernel computes
 * the listed pixels' fine samples in the wide number system, one lane per sample, with the table's skips under MBK_DEEP_XBLA
 * (an orbit of length 1 has no table: the flag changes nothing).  The ctx keeps TWO wide tables beside each orbit copy (see
 * "Extended-range deep views with bilinear approximation"); a render with the flag acquires the base view's and the fine
 * view's together before it enqueues anything, and neither takes the other's place (equal dcmax: one table).  A first call
 * with a given (orbit, view, s) may therefore upload the wide orbit table and build and upload the tables synchronously; after
 * it the launch form performs no host synchronisation for as long as both tables stay resident -- until a launch on the same
 * orbit brings a third dcmax -- and can be captured into a graph ("Graph capture", as above).
 *
 * MBK_ERR_INVALID, with nothing written: whatever mbk_deep_xview_render_* refuses for MBK_RENDER_SMOOTH, any other source,
 * threshold > 256, any flag but MBK_DEEP_XBLA (MBK_DEEP_BLA in the words of mbk_deep_xview_launch).  d_mask / h_mask may be
 * NULL.
 *
 * Out of scope: Julia views; the equalised, bytes and distance sources; a distance-guided criterion; sharding and slot forms.
 */
int mbk_deep_xview_render_adaptive_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *d_rgba,
                                          uint8_t *d_mask, void *hip_stream);
int mbk_deep_xview_render_adaptive_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, uint32_t threshold, uint8_t *h_rgba,
                                           uint8_t *h_mask, mbk_stats *stats);

/*
 * Count histograms and histogram-equalised colouring.  NOT in the reference; additive (the ABI version stays 5): no existing
 * call changes.  Every colouring above maps a sample to a palette position through a scale and an offset the caller must
 * already know; a deep view's escaped counts lie in a narrow, unknown interval far from 0.  A histogram of the view's counts,
 * built on the device, tells the caller the range (8 mrd bytes cross PCIe instead of 12 per pixel), and a cumulative table
 * made from it spreads the palette evenly over the samples that are there.
 *
 * Contract (exact; tests/histogram_model.py restates it in numpy, tests/test_histogram.py and tests/test_gpu_histogram.py hold
 * the host and the GPU to it):
 *   histogram  hist is uint64[mrd], 1 <= mrd <= MBK_HISTOGRAM_MAX_MRD (an 8 MiB table); hist[c] is the number of samples whose
 *              count is c (counts lie in {0} U [1, mrd - 1]).  A count outside [0, mrd - 1] is skipped, and nothing is ever
 *              written outside the mrd bins.  hist[0] is mbk_stats.never_pixels, and sum c hist[c] + (mrd - 1) hist[0] is
 *              mbk_stats.pixel_iterations.  Integer sums: exact whatever the schedule.
 *   table      lut is double[mrd + 2].  With E = sum_{c >= 1} hist[c], cum(k) = sum_{1 <= c < min(k, mrd)} hist[c] and
 *              h(k) = hist[k] for 1 <= k < mrd, else 0:  lut[0] = 0, and for k >= 1
 *                lut[k] = fl((2 cum(k - 1) + h(k - 1)) / (2 E)),
 *              the share of escaped samples with a lower count plus half the share with count k - 1 (nu of a count-n sample
 *              lies in about (n + 0.16, n + 1.53]).  Monotone, lut[1] = 0, lut[mrd + 1] = 1.  E = 0 gives all zeros.  2 E must
 *              be below 2^53, so that the conversions are exact and there is one correctly rounded division.  Count 0, the
 *              interior, takes no part.
 *   value      of a sample with smooth value nu, every operation rounded on its own: x = nu, or 0 unless 0 <= x (negative,
 *              -inf, NaN).  If x >= mrd + 1: v = lut[mrd + 1].  Otherwise k = floor(x), f = x - k (exact) and
 *              v = fl(lut[k] + fl(f fl(lut[k + 1] - lut[k]))).
 *   colour     MBK_RENDER_EQUALIZED: `inside` if the sample's count is 0; otherwise v as above, then the MBK_RENDER_DISTANCE
 *              rule with v in place of de: t = fl(fl(v scale) + offset), no wrap, t >= n - 1 gives the last entry.
 *              2 <= palette_len <= 65536; scale and offset take the MBK_RENDER_SMOOTH ranges (scale = n - 1, offset = 0
 *              spreads the whole palette).  Samples, banding, flags and resolve are those of MBK_RENDER_SMOOTH.
 *
 * mbk_counts_histogram: asynchronous, over counts already in HBM (the sibling of mbk_reduce_counts), on the caller's stream.
 * It ADDS into d_hist (8-byte aligned; d_counts 4-byte aligned): the caller clears it, so that windows, bands and GPUs can
 * accumulate into one table.  n == 0 is a no-op.
 * mbk_view_histogram_launch / mbk_deep_view_histogram_launch: the window's counts are produced by mbk_view_launch /
 * mbk_deep_view_launch into scratch the ctx keeps per stream (the renders' sample scratch), with the same kernel selection and
 * refusal rules: `flags` carries kernel selection and MBK_PRECISION_F32 for a plain view, MBK_DEEP_BLA alone for a deep one, MBK_DEEP_XBLA alone for an
 * extended-range one.  4 bytes per
 * sample, banded under MBK_RENDER_BAND_BYTES exactly as a render bands, so no view size needs more scratch.  Each band's
 * counts are ADDED into d_hist.
 * _compute: synchronous on slot 0 (the slot-0 rule applies); h_hist is OVERWRITTEN, not accumulated; stats as for
 * mbk_view_compute without bytes (kernel_ms from the first sample kernel to the last histogram kernel, d2h_ms the copy of the
 * table, pixel_iterations and never_pixels from the existing reduction over the same counts -- not from the table).
 * The _host forms need no ctx and no device.  mbk_counts_histogram_host ADDS, like the device call.  mbk_equalize_value_host
 * returns 0 for a NULL table or an mrd above the limit.
 * MBK_ERR_INVALID, with nothing written: NULL pointers, mrd == 0 or above MBK_HISTOGRAM_MAX_MRD, misaligned device pointers,
 * a total at or above 2^52 escaped samples (mbk_equalize_lut_host), and whatever the sample launches refuse.
 *
 * mbk_*_render_equalized_*: the arguments of the four render calls plus the table.  h_lut is a HOST pointer to lut_len entries,
 * copied during the call into scratch the ctx keeps per stream, under the palette's wait-on-change rule.  They accept
 * MBK_RENDER_EQUALIZED only.  MBK_ERR_INVALID, with nothing written: whatever the render calls refuse for MBK_RENDER_SMOOTH,
 * any other source, a NULL h_lut, lut_len != mrd + 2 (so mrd <= MBK_HISTOGRAM_MAX_MRD), an entry that is not finite or lies
 * outside [0, 1].  mbk_render_resolve_equalized_host is the host twin of the resolve (mrd = lut_len - 2), compiled from the
 * same colour function as the kernel.
 *
 * The histogram kernel (csrc/mbk_histogram.h has the design and what was measured): zeros are counted in registers, a
 * workgroup keeps a window of bins in LDS where its first samples say the counts lie, equal values are folded within a wave
 * before any atomic, and what falls outside the window goes to the table with 64-bit global atomics.
 *
 * Out of scope: fusing the histogram into the escape kernels; histograms of nu itself or of distance values; byte histograms
 * of stored chunks (render_level); a sharding form (the additive d_hist makes one easy); slot / submit forms.
 */
#define MBK_HISTOGRAM_MAX_MRD (1u << 20)
int mbk_counts_histogram(mbk_ctx *ctx, const int32_t *d_counts, uint64_t n, uint32_t mrd, uint64_t *d_hist, void *hip_stream);
int mbk_view_histogram_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint64_t *d_hist,
                              void *hip_stream);
int mbk_deep_view_histogram_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                   uint32_t flags, uint64_t *d_hist, void *hip_stream);
int mbk_view_histogram_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint64_t *h_hist,
                               mbk_stats *stats);
int mbk_deep_view_histogram_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                    uint32_t flags, uint64_t *h_hist, mbk_stats *stats);
/* The same for an extended-range deep view (the counts of mbk_deep_xview_launch; every flag is MBK_ERR_INVALID). */
int mbk_deep_xview_histogram_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                    uint32_t flags, uint64_t *d_hist, void *hip_stream);
int mbk_deep_xview_histogram_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                     uint32_t flags, uint64_t *h_hist, mbk_stats *stats);
int mbk_counts_histogram_host(const int32_t *counts, uint64_t n, uint32_t mrd, uint64_t *hist);
int mbk_equalize_lut_host(const uint64_t *hist, uint32_t mrd, double *lut);
double mbk_equalize_value_host(const double *lut, uint32_t mrd, double nu);
int mbk_view_render_equalized_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                                     const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len, uint8_t *d_rgba,
                                     void *hip_stream);
int mbk_view_render_equalized_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                                      const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len, uint8_t *h_rgba,
                                      mbk_stats *stats);
int mbk_deep_view_render_equalized_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                          uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                          uint8_t *d_rgba, void *hip_stream);
int mbk_deep_view_render_equalized_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                           uint8_t *h_rgba, mbk_stats *stats);
int mbk_deep_xview_render_equalized_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                           uint8_t *d_rgba, void *hip_stream);
int mbk_deep_xview_render_equalized_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                            uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                            uint8_t *h_rgba, mbk_stats *stats);
int mbk_render_resolve_equalized_host(const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len, uint32_t width,
                                      uint32_t height, const int32_t *counts, const double *smooth, uint8_t *rgba);

/*
 * Julia views.  NOT in the reference; additive (the ABI version stays 5): no existing call changes.  Every view above iterates
 * z -> z^2 + c with the pixel as c.  A Julia view fixes c = (c_r, c_i) and takes the pixel as the starting point: "the Julia set
 * of the point I am looking at".  A Julia view is an mbk_view plus the parameter; coordinates (np.linspace), window rule,
 * layout and row order are those of every view.
 *
 * Contract (exact; tests/julia_model.py restates it in numpy, tests/test_julia.py and tests/test_gpu_julia.py hold the host
 * and the GPU to it):
 *   state     for the pixel with coordinate p, z_0 = p.  z_0 is never tested (as calc_mb_value never tests its z_0 = c).
 *   step      z_(k+1) = z_k^2 + c in binary64, every operation rounded on its own, in the reference's order:
 *               zr' = fl(fl(fl(zr zr) - fl(zi zi)) + c_r),  zi' = fl(fl(fl(2 zr) zi) + c_i);   at most mrd - 1 updates;
 *               mag_k = fl(fl(zr^2) + fl(zi^2)).
 *   count     n = the first k >= 1 with mag_k >= 4 (false for NaN), 0 if there is none.  mrd 0 and 1 run no step.
 *   outputs   bytes: the quantiser of every view, of n.  smooth: nu = n + 1 - log2(0.5 ln mag_n), the function and the
 *             allowance of mbk_view_launch_smooth (2.57 ulp(nu) + 3.38 x 2^-52 around the correctly rounded value at mag_n).
 *             mbk_stats means what it means for mbk_view_compute.
 *   identity  at a pixel whose coordinate equals c bit for bit, n is the Mandelbrot count of c (the same orbit).
 *   windows   a window of a view is bit-identical to that part of the whole view.
 *   odd input coordinates whose squares overflow or turn NaN store whatever this strict evaluation stores.
 *
 * Two exactness rules, both decided on the host once per launch (c is uniform):
 *   doubling  The kernels form zi' as fma(2, fl(zr zi), c_i), which equals the literal form unless zr zi is a non-zero
 *             subnormal (2 fl(zr zi) then carries a rounding that fl(fl(2 zr) zi) does not).  For a Mandelbrot view that
 *             hazard sits on rows with a tiny c_i.  For a Julia view zi is NOT tied to c_i: with c_i = 0 (c = -1, -0.75,
 *             0.25 ...) a row whose z0_i is tiny keeps zi tiny for many steps.  |c_i| >= 2^-900 makes the rewrite safe for
 *             every z: both candidate addends are below 2^-1021, less than a quarter ulp of c_i, and round away alike.  So
 *             every launch with |c_i| < 2^-900, c_i = 0 included, takes the literal 8-operation per-step loop.  (The two forms
 *             also part where fl(2 zr) overflows and zi = 0: NaN against c_i.  Only z_0 can do that -- a later |zr| >= 2^512 has
 *             mag = inf and has escaped --, and a view's coordinates are bounded by 2^500; mbk_julia_count_host, which takes any
 *             z, uses the literal form beyond that bound.)
 *   grouping  The grouped bailout test (MBK_KERNEL_GROUP) relies on "|z|^2 >= 4 stays >= 4", which holds for
 *             |c|^2 < 4 - 1e-9 whatever z is (|z'| >= |z|^2 - |c| > 2 + 2e-10) and fails above: for |c| > 2 a |z| >= 2
 *             that is below |c| can come back inside.  A launch whose fl(fl(c_r^2) + fl(c_i^2)) is not below 4 - 1e-9 takes
 *             the per-step loop throughout.  The cycle test needs only that the step is a function of the state, which a
 *             fixed c gives it.
 *
 * flags: MBK_WANT_COUNTS | MBK_WANT_BYTES on the three view calls, plus kernel selection: MBK_KERNEL_DEFAULT (the library's
 * choice: the grouped test with the cycle test where the two rules allow it), MBK_KERNEL_ASM (the per-step loop, every
 * iteration executed: the witness), MBK_KERNEL_GROUP (grouped test + cycle test under MBK_OPT_GROUP_STEPS, _EXACT_STEPS,
 * _CYCLE_DETECT, _CYCLE_WINDOW and _WAVE_LIMIT; no other option is consulted; _WAVE_LIMIT's cap, unused LDS per workgroup,
 * holds for this kernel as for any: its registers allow 8 waves per SIMD, so they never bind before it).  Every accepted value gives identical output.
 * MBK_ERR_INVALID, with nothing written: MBK_KERNEL_SIMPLE / _REFILL / _SCAN, MBK_PRECISION_F32, MBK_LAZY_UNIFORM, any other
 * flag bit, a non-finite c, mrd >= 2^31, mrd == 0 with bytes, no output selected, a wanted output with a NULL pointer, and
 * whatever mbk_view_launch refuses of a view.
 *
 * mbk_julia_view_launch: asynchronous, device pointers, the caller's stream; d_smooth may be NULL.  _compute: synchronous on
 * slot 0, host pointers, h_smooth may be NULL.  _submit: on a slot, completed by mbk_wait.
 * mbk_julia_view_render_* / _render_equalized_* / _histogram_*: the calls of the same names without "julia_", on the Julia
 * samples: banding, palettes, supersampling, tables and statistics are the same code.  flags carry kernel selection only;
 * sources MBK_RENDER_BYTES, _SMOOTH and (equalized calls) _EQUALIZED; the distance sources are refused.
 * mbk_julia_count_host: one orbit on the host, no ctx, no device -- the contract's loop as the kernels restate it, with the
 * doubling a launch with this c would use.  *mag (may be NULL) is the mag of the last step run (mag_n if n > 0; 0 if no step
 * ran).  MBK_ERR_INVALID for a NULL count, a non-finite c, mrd >= 2^31; z may be anything.
 *
 * Distance estimates are calls of their own: "Distance estimates for Julia views", below.
 *
 * Out of scope: deep (perturbation) Julia views, an fp32 form, the scan / refill / units machinery, the z -> -z symmetry.
 */
int mbk_julia_view_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                          int32_t *d_counts, uint8_t *d_bytes, double *d_smooth, void *hip_stream);
int mbk_julia_view_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                           int32_t *h_counts, uint8_t *h_bytes, double *h_smooth, mbk_stats *stats);
int mbk_julia_view_submit(mbk_ctx *ctx, int slot, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                          int32_t *h_counts, uint8_t *h_bytes);
int mbk_julia_view_render_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                 const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_julia_view_render_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                  const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_julia_view_render_equalized_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd,
                                           uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                           uint8_t *d_rgba, void *hip_stream);
int mbk_julia_view_render_equalized_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd,
                                            uint32_t flags, const mbk_render_spec *spec, const double *h_lut, uint32_t lut_len,
                                            uint8_t *h_rgba, mbk_stats *stats);
int mbk_julia_view_histogram_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                    uint64_t *d_hist, void *hip_stream);
int mbk_julia_view_histogram_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                     uint64_t *h_hist, mbk_stats *stats);
int mbk_julia_count_host(double z_r, double z_i, double c_r, double c_i, uint32_t mrd, int32_t *count, double *mag);

/*
 * Distance estimates for Julia views.  NOT in the reference; additive (the ABI version stays 5): no existing call changes what
 * it stores or refuses.  The exterior distance estimate began with Julia sets: for a fixed c the derivative of the orbit with
 * respect to its STARTING POINT is carried along, and the pixel reports
 *     de = 2 |z| ln |z| / |d|,   d = dz_k / dz_0,
 * a length in the complex plane within a known factor of the true distance from p to the Julia set of c (Koebe: between
 * about de / 4 and de for a connected set).  Dendrites and Cantor dusts (c = i, c = -0.8 + 0.156i) are thinner than any pixel
 * and every sample of them escapes; this is the output that shows them.
 *
 * Contract (tests/julia_distance_model.py restates it in numpy; tests/test_julia_distance.py and
 * tests/test_gpu_julia_distance.py hold the host twin and the GPU to it).  For a pixel with coordinate p of an mbk_view and a
 * parameter c = (c_r, c_i), binary64, every operation rounded on its own, no contraction:
 *   state     z_0 = p, d_0 = (1, 0).  Step k -> k + 1:
 *               u = fl(fl(zr dr) - fl(zi di)), v = fl(fl(zr di) + fl(zi dr))   both from z_k and d_k
 *               d' = (2u, 2v)     both doublings are exact, subnormals included; an overflow is the infinity IEEE gives.  There
 *                                 is no "+ 1": that term of "Distance estimates" is dc/dc, and here c does not move.
 *               z_(k+1) by the recurrence of "Julia views", unchanged, with the doubling a count launch with this c takes
 *               (|c_i| < 2^-900: the literal form; otherwise fma(2, fl(zr zi), c_i), the same bits there).
 *   count     n is exactly the count of mbk_julia_view_launch: the first k >= 1 with mag_k >= 4, 0 if none, at most mrd - 1
 *             updates.
 *   run-on    a pixel with n > 0 runs on, uncounted, with both recurrences until mag >= 2^32 or 64 further steps have run: the
 *             constant pair of "Distance estimates".  For |c| > 2 mag may fall below 4 again during the run-on; that changes
 *             nothing: n stays, and the steps go on.
 *   output    de = the output expression of "Distance estimates" (the same function, shared) at the final state, with
 *             dmag = fl(fl(dr^2) + fl(di^2)): 0 for n = 0, 0 instead of NaN, infinities as IEEE gives them.  The allowance
 *             against the correctly rounded value is measured on Julia pairs (tests/julia_distance_model.py: J0 for the host,
 *             J0 + 1 for the device).
 *   critical  the one case plain views do not have: a z_0 that is exactly 0 -- the critical point -- has d_1 = 2 z_0 d_0 = 0 and
 *   point     so d_k = 0 for every k >= 1.  With n > 0 its dmag is 0 and it stores +inf.  (The centre pixel of the 65 x 65 view
 *             of [-2, 2]^2 with c = (0.285, 0.01), mrd = 500: n = 19, dmag = 0, de = +inf, the only infinity in that view.)  A
 *             view with an odd number of samples on both axes, centred on 0, holds that pixel; colour rules that clamp
 *             (MBK_RENDER_DISTANCE: the last palette entry) take it in their stride.
 *   mrd       0 and 1 run no step: every count and de is 0.
 *   windows   a window is bit-identical to the same pixels of the whole view.
 *
 * Two designs, selected by the kernel bits of `flags`, bit-identical in what they store:
 *   MBK_KERNEL_DEFAULT / _GROUP   two passes: mbk_julia_view_launch with that selector writes the counts (grouped test and
 *             cycle test as its own two rules decide), then a derivative pass runs each pixel with n > 0 for exactly n steps
 *             without a bailout test, plus the run-on.  A block whose counts are all 0 -- the whole interior of a connected
 *             set -- stores zeros after one load.  With d_counts == NULL the counts live in the per-stream scratch of
 *             mbk_view_launch_distance.
 *   MBK_KERNEL_ASM                one pass: the derivative rides in a per-step escape loop; no counts are read.
 * mbk_julia_view_launch_distance: asynchronous, DEVICE pointers (window-sized, nothing is written outside them), the caller's
 * stream.  _compute_distance: synchronous into HOST buffers on slot 0; stats as for mbk_view_compute_distance (the run-on
 * steps are not in pixel_iterations).  The counts pointer may be NULL in both.
 * mbk_julia_view_distance_render_launch / _compute: the render calls on these samples, calls of their own as the other
 * distance renders are.  The source must be MBK_RENDER_DISTANCE; colour rule, supersampling, banding, statistics and every
 * other refusal are those of mbk_view_render_* with that source.  mbk_julia_view_render_* keeps refusing the distance sources.
 * mbk_julia_distance_host: one orbit on the host, no ctx, no device, compiled from the step function the kernels use, with
 * the doubling a launch with this c would use (and the literal one for |z_r| > 2^500, as mbk_julia_count_host).  It returns the
 * final state: *count = n, *extra = the run-on steps taken, z, d, mag, dmag and de (the host's ln).  Every output pointer but
 * count may be NULL; z may be anything.
 *
 * MBK_ERR_INVALID, with nothing written: MBK_KERNEL_SIMPLE / _REFILL / _SCAN; MBK_PRECISION_F32, MBK_LAZY_UNIFORM, MBK_DEEP_BLA,
 * MBK_DEEP_XBLA and any other flag bit; a non-finite c; mrd >= 2^31; a NULL distance or rgba pointer; whatever
 * mbk_julia_view_launch refuses in a view; in the render calls every source but MBK_RENDER_DISTANCE; in the host twin a NULL
 * count.
 *
 * Out of scope: deep (perturbation) Julia views, Julia interior views, a sharding form, slot / submit forms, the z -> -z
 * symmetry.
 */
int mbk_julia_view_launch_distance(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                   int32_t *d_counts, double *d_distance, void *hip_stream);
int mbk_julia_view_compute_distance(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                    int32_t *h_counts, double *h_distance, mbk_stats *stats);
int mbk_julia_view_distance_render_launch(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                          const mbk_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_julia_view_distance_render_compute(mbk_ctx *ctx, const mbk_view *view, double c_r, double c_i, uint32_t mrd, uint32_t flags,
                                           const mbk_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_julia_distance_host(double z_r, double z_i, double c_r, double c_i, uint32_t mrd, int32_t *count, int32_t *extra,
                            double *zr, double *zi, double *dr, double *di, double *mag, double *dmag, double *de);

/*
 * Density views (Buddhabrot / Nebulabrot).  NOT in the reference; additive (the ABI version stays 5): no existing call changes.
 * Every picture above colours a pixel by what happened to that pixel's own orbit.  A density view instead counts where the
 * orbits of the escaping samples GO: each orbit point adds one to the cell of a 2-D table it falls into.  The orbit points
 * never leave the kernels, so this is the one picture a caller cannot assemble from the other calls' outputs.
 *
 * Contract (exact; tests/density_model.py restates it in numpy, tests/test_density.py and tests/test_gpu_density.py hold the
 * host twins and the GPU to it):
 *   samples   the pixels of an mbk_view, the sample view, window semantics as everywhere: the coordinates are those of
 *             mbk_view_launch, bit for bit, and so is the count n of each sample (mrd as usual).  A sample QUALIFIES when
 *             min_count <= n <= max_count, with 1 <= min_count and max_count == 0 meaning mrd - 1.  n = 0 (the sample never
 *             escapes) never qualifies.
 *   deposits  a qualifying sample deposits its orbit points z_0 = c, z_1, ..., z_(n-1): n points, all those before the step that
 *             tripped `>= 4`.  The points are the reference's recurrence in binary64, every operation rounded on its own, in its
 *             literal form:  zr' = fl(fl(fl(zr zr) - fl(zi zi)) + c_r),  zi' = fl(fl(fl(2 zr) zi) + c_i).  z_0 may lie anywhere
 *             (a sample far outside |c| = 2 has n = 1 and deposits c alone).
 *   target    a second rectangle (start_r, start_i, range_r, range_i) cut into width x height CELLS, W, H >= 1,
 *             W H <= MBK_DENSITY_MAX_CELLS, starts finite, ranges finite and > 0.  Cells are half-open; they are not linspace
 *             samples.  With inv_r = fl(W / range_r) and inv_i = fl(H / range_i), computed once, the cell of a point is, in
 *             binary64 with every operation rounded on its own:
 *               tx = fl(fl(zr - start_r) inv_r),  ty = fl(fl(zi - start_i) inv_i);
 *               the point lands in cell (floor(tx), floor(ty)) iff 0 <= tx < W and 0 <= ty < H, otherwise it is DROPPED.
 *             The comparisons are false for NaN (and an inv_* that overflowed drops or keeps a point as IEEE arithmetic says).
 *             A point exactly on the right or the top edge is outside.  Row 0 is the lowest imaginary part.
 *   table     uint32[H][W] on the device, cell (x, y) at word y W + x.  A launch ADDS to it, modulo 2^32; the caller clears it,
 *             as for mbk_counts_histogram.  Integer sums: the table is exact whatever the schedule, and windows and bands of the
 *             sample view, several launches and several GPUs sum to the whole view's table.  Nothing is ever written outside
 *             the W H words.
 *   mrd       0 and 1 run no step: nothing is deposited (max_count == 0 is accepted and stands for "every escaped sample").
 *
 * mbk_view_density_launch: asynchronous, on the caller's stream; d_density is a DEVICE table, 4-byte aligned.  `flags` carries
 * kernel selection for the count pass only.  Two passes, like the default distance path: the window's counts come from
 * mbk_view_launch with that selector, cycle test and all (for a density view the interior samples are pure waste, and the count
 * kernels retire them for nearly nothing), into the sample scratch the ctx keeps per stream -- 4 bytes per sample, banded under
 * MBK_RENDER_BAND_BYTES exactly as a histogram bands; then a replay kernel (csrc/mbk_density.h) runs each qualifying sample for
 * exactly n steps without a bailout test and issues one 32-bit global atomic add per point inside the target.
 * mbk_view_density_compute: synchronous on slot 0 (the slot-0 rule applies); h_density (W H words) is OVERWRITTEN, not accumulated;
 * stats (may be NULL) as for mbk_view_compute without bytes, over the samples (kernel_ms from the first count kernel to the last
 * replay kernel, d2h_ms the copy of the table); dstats (may be NULL): the points deposited and the points dropped, which add up
 * to the sum of n over the qualifying samples -- when every escaped sample qualifies,
 * pixel_iterations - (mrd - 1) never_pixels.
 * mbk_density_max: a device reduction over n cells of a DEVICE table on the caller's stream, then a wait for that stream: the
 * largest cell and the sum of all cells, so that a caller can choose a scale without copying the table.  n == 0 gives 0, 0.
 * mbk_density_render_launch / _compute: a table of width x height cells as an RGBA8 image of (width / k) x (height / k) pixels
 * through the caller's palette.  A cell v becomes g(v) = v (MBK_DENSITY_LINEAR) or g(v) = fl(sqrt(v)) (MBK_DENSITY_SQRT; v is
 * exact in binary64 and the square root correctly rounded, so g is the same on the host and on the device), then
 * t = fl(fl(g scale) + offset) and a colour by the MBK_RENDER_DISTANCE rule: no wrap, the last entry from t >= n - 1 up, t = 0
 * unless 0 <= t; 2 <= palette_len <= 65536, 0 < scale <= 2^80, |offset| <= 2^20.  factor k in {1, 2, 4, 8} is a box filter over
 * k x k cells, applied to the colours with the "resolve" rule of the Rendering section; width and height must be multiples of k.
 * _launch reads a DEVICE table and writes a DEVICE image on the caller's stream (both 4-byte aligned); the palette upload
 * follows the renders' wait-on-change rule.  _compute takes a HOST table, uploads it, and returns the image in a HOST buffer,
 * synchronously on slot 0; stats: kernel_ms of the resolve, d2h_ms of the image, the other fields 0.
 * The _host forms need no ctx and no device; they are compiled from the functions the kernels use.  mbk_density_cell_host: one
 * point -> *inside = 1 and its cell, or *inside = 0.  mbk_density_accumulate_host: the whole contract for a view / window, ADDED
 * into density (one orbit at a time: for the CPU tests, small views only).  mbk_density_resolve_host: the render.
 * MBK_ERR_INVALID, with nothing written: NULL pointers (stats and dstats excepted); a misaligned device table or image;
 * min_count == 0; min_count > max_count after the max_count == 0 substitution; max_count >= mrd when mrd >= 2; mrd >= 2^31; a
 * target or a render spec outside the limits above; any flag but kernel selection (MBK_PRECISION_F32, MBK_LAZY_UNIFORM,
 * MBK_DEEP_BLA, MBK_WANT_*); the kernels mbk_view_launch_smooth refuses (MBK_KERNEL_SIMPLE, MBK_KERNEL_REFILL); and whatever
 * mbk_view_launch refuses in a view.
 *
 * mbk_density_build_info: host-only, needs no ctx: which form of the replay this library was compiled with -- 0, the plain form
 * (one lane per sample in image order; what ships), or 1, the compacted list (-DMBK_DENSITY_COMPACT=1, csrc/mbk_density.h).  The
 * two forms compute the same tables; a test that loads a second build asks here which one it got.
 *
 * Out of scope: deep, Julia and fp32 forms; the anti-Buddhabrot (orbits of the samples that never escape); random or jittered
 * sampling; the z -> conj(z) symmetry; fusing the deposits into the count kernels; 64-bit tables; an equalised colouring of
 * densities.
 */
#define MBK_DENSITY_MAX_CELLS (1u << 28)
#define MBK_DENSITY_LINEAR 0u
#define MBK_DENSITY_SQRT 1u
typedef struct mbk_density_target {
    double start_r, start_i;
    double range_r, range_i;
    uint32_t width, height;
} mbk_density_target;
typedef struct mbk_density_stats {
    uint64_t deposits; /* orbit points that landed in a cell */
    uint64_t dropped;  /* orbit points of qualifying samples that fell outside the target */
} mbk_density_stats;
typedef struct mbk_density_render_spec {
    uint32_t mode;          /* MBK_DENSITY_LINEAR | MBK_DENSITY_SQRT */
    uint32_t factor;        /* k: 1, 2, 4, 8 */
    const uint8_t *palette; /* HOST pointer, palette_len x RGBA8; copied during the call */
    uint32_t palette_len;
    double scale, offset;
} mbk_density_render_spec;
int mbk_view_density_launch(mbk_ctx *ctx, const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                            uint32_t max_count, uint32_t flags, uint32_t *d_density, void *hip_stream);
int mbk_view_density_compute(mbk_ctx *ctx, const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                             uint32_t max_count, uint32_t flags, uint32_t *h_density, mbk_stats *stats, mbk_density_stats *dstats);
int mbk_density_max(mbk_ctx *ctx, const uint32_t *d_density, uint64_t n, uint32_t *max, uint64_t *total, void *hip_stream);
int mbk_density_render_launch(mbk_ctx *ctx, const uint32_t *d_density, uint32_t width, uint32_t height,
                              const mbk_density_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_density_render_compute(mbk_ctx *ctx, const uint32_t *h_density, uint32_t width, uint32_t height,
                               const mbk_density_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_density_cell_host(const mbk_density_target *target, double z_r, double z_i, uint32_t *cell_x, uint32_t *cell_y, int *inside);
int mbk_density_accumulate_host(const mbk_view *view, const mbk_density_target *target, uint32_t mrd, uint32_t min_count,
                                uint32_t max_count, uint32_t *density, mbk_density_stats *dstats);
int mbk_density_resolve_host(const mbk_density_render_spec *spec, uint32_t width, uint32_t height, const uint32_t *density,
                             uint8_t *rgba);
int mbk_density_build_info(void);

/*
 * Interior views: periods and interior distance estimates.  NOT in the reference; additive (the ABI version stays 5): no
 * existing call changes.  Every output above is about the outside of the set; a pixel that never escapes is "count 0" and
 * nothing more.  An interior view says which component such a pixel lies in -- the period of the attracting cycle its orbit
 * settles on -- and how far inside it is: the interior distance estimate, which Koebe's theorem holds to
 * true distance <= de <= 4 x true distance.
 *
 * The cycle test of the count kernels cannot give the period: the bitwise period of a settled binary64 orbit is usually a
 * proper multiple of the mathematical one (inside the main cardioid it reads 1, 2, 3, ... 98).  The contract therefore
 * reduces the bitwise period with a tolerance.
 *
 * Contract (exact; tests/interior_model.py restates it in numpy, tests/test_interior.py and tests/test_gpu_interior.py hold the
 * host twin and the GPU to it).  For the pixel with coordinate c of a plain mbk_view, in binary64, every operation rounded on
 * its own.  step(z) is the recurrence of mbk_view_launch, unchanged; cmul(a, b) = (fl(fl(ar br) - fl(ai bi)),
 * fl(fl(ar bi) + fl(ai br))); complex sums are componentwise; doublings are multiplications by 2.
 *   count       n is exactly the count of mbk_view_launch.  A pixel with n > 0 stores period 0 and de 0.
 *   cycle       for n = 0.  z_0 = c, reference r = z_0, window w = 1, since = 0.  For k = 1 .. mrd - 1: z_k = step(z_(k-1)),
 *               since += 1; if both 64-bit patterns of z_k equal those of r (a bit compare: -0 != +0), L = since and the
 *               search stops -- this is tested first; otherwise, if since == w: r = z_k, w = 2 w, since = 0.  No hit within
 *               the mrd - 1 updates: the pixel is UNKNOWN, period 0 and de 0.  The schedule (w, since) is the same for every
 *               pixel; L is Brent's minimal bitwise period and r lies on the cycle.
 *   period      y_0 = r, y_d = step(y_(d-1)) for d = 1 .. L; p is the first d with
 *               max(|fl(yr_d - rr)|, |fl(yi_d - ri)|) <= 2^-40.  d = L always qualifies.  The constant is part of the contract.
 *   derivatives p steps from z = r with A = (1, 0) (dz), B = 0 (dc), E = 0 (dzz), F = 0 (dcz), every update from the old values:
 *                 F' = 2 (cmul(z, F) + cmul(A, B)),  E' = 2 (cmul(A, A) + cmul(z, E)),
 *                 B' = 2 cmul(z, B) + (1, 0) with the real part fl(2u + 1) as in "Distance estimates",
 *                 A' = 2 cmul(z, A),  z' = step(z).
 *   output      m2 = fl(fl(Ar^2) + fl(Ai^2)).  If not m2 < 1: de = 0, and the period stays p.  Otherwise g = (fl(1 - Ar), -Ai),
 *               h = cmul(E, B), t = cmul(h, conj g), gm = fl(fl(gr^2) + fl(gi^2)), G = F + (fl(tr / gm), fl(ti / gm)),
 *               den = fl(fl(Gr^2) + fl(Gi^2)) and de = fl(fl(1 - m2) / fl(sqrt(den))).  Division and square root are the
 *               correctly rounded ones; there is no libm call, so host and device agree to the bit.  Never NaN and never
 *               negative: 0 is stored where the expression is NaN; den = 0 gives +inf as IEEE does.  de is a length in the
 *               complex plane, the unit of mbk_view_launch_distance.
 *   mrd         0 and 1 run no step: everything is 0.  mrd >= 2^31 is refused.
 * Windows of a view are bit-identical to the whole view.
 * By hand: c = (0, 0) gives 0, 1, 0.5; c = (-1, 0) gives 0, 2, 0.25 from mrd 4 on and is unknown at mrd 3.
 *
 * Held to the mathematics (tests/interior_truth.py, tests/test_interior_truth.py; on the device in tests/test_gpu_interior.py):
 * de is meant to be (1 - |lambda|^2) / |d lambda / dc|, lambda(c) the multiplier of the attracting cycle.  The tests evaluate that
 * with mpmath at 256 bits from the pixel's coordinate and its period alone -- Newton on the p-fold map, d lambda / dc by central
 * differences -- and require of every settled pixel that p is the exact minimal period of the cycle, that |lambda| < 1, and that
 * |de - de_true| / de_true <= K0 p 2^-52 / (1 - |lambda|^2) with K0 = 69, the worst figure measured (a period-3 pixel at
 * |lambda| = 0.84).  The analytic |F + E B / (1 - A)| in exact arithmetic agrees with the finite difference to 1e-30.
 *
 * Two passes (csrc/mbk_interior.h): the counts come from the count kernels mbk_view_launch would run for the selector, cycle test
 * and all, into d_counts or scratch the ctx keeps per stream; then one lane per count-0 pixel runs the four stages.
 * mbk_view_interior_launch: asynchronous, DEVICE pointers on the caller's stream (window-sized buffers; nothing is written
 * outside them; no statistics).  d_counts may be NULL; one of d_period / d_distance may be NULL, not both.
 * mbk_view_interior_compute: synchronous into HOST buffers on slot 0 (the slot-0 rule applies), the same pointer rules, stats as
 * for mbk_view_compute_distance.
 * `flags` carries kernel selection only: MBK_KERNEL_DEFAULT, _SCAN and _GROUP, bit-identical.  MBK_ERR_INVALID, with nothing
 * written: MBK_KERNEL_ASM / _SIMPLE / _REFILL, MBK_PRECISION_F32, MBK_LAZY_UNIFORM, MBK_DEEP_BLA, any other flag bit, both value
 * pointers NULL, mrd >= 2^31 and whatever mbk_view_launch refuses in a view.
 * mbk_interior_host: one pixel on the HOST, compiled from the functions the kernel uses: no ctx, no device.  *cycle_len is L
 * (0 for an escaping or an unknown pixel).  Every out pointer but count may be NULL.  MBK_ERR_INVALID for a NULL count and
 * mrd >= 2^31.
 *
 * Interior renders are calls of their own, not an MBK_RENDER_* source.  Colour of a sample: `outside` if n > 0; `unknown` if it
 * has no period; otherwise base = p[(period - 1) mod n], 1 <= n <= 65536, t = fl(de scale), f = 256 where t >= 1 (+inf
 * included) and floor(256 t) below, each of R, G, B (base f + 128) >> 8, alpha the base's.  0 < scale <= 2^80, finite:
 * scale = 2^80 is the flat period map, scale = 1 / (k pitch) darkens the inner k pixels towards the boundary.  Samples (16 bytes:
 * count, period, de), supersampling set, resolve, output layout, banding under MBK_RENDER_BAND_BYTES, the palette's
 * wait-on-change rule and the statistics of _compute are those of "Rendering"; flags as for mbk_view_interior_launch.
 * mbk_interior_resolve_host: colour and resolve on the HOST for caller-supplied samples of (width s) x (height s).
 *
 * Out of scope: deep, extended-range and Julia views; sharding and slot forms; compacting the unknown pixels into full waves;
 * a Newton search for the unknown pixels near the boundary.
 */
typedef struct mbk_interior_render_spec {
    uint32_t supersample;   /* 1, 2, 3, 4, 8 */
    const uint8_t *palette; /* HOST pointer, palette_len x RGBA8, entry k the colour of period k + 1; copied during the call */
    uint32_t palette_len;   /* 1 .. 65536 */
    uint8_t unknown[4];     /* a sample that never escapes and shows no cycle within mrd */
    uint8_t outside[4];     /* a sample that escapes */
    double scale;
    uint32_t max_band_rows; /* 0 = the library's choice; any value gives the same image */
} mbk_interior_render_spec;
int mbk_view_interior_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *d_counts,
                             int32_t *d_period, double *d_distance, void *hip_stream);
int mbk_view_interior_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *h_counts,
                              int32_t *h_period, double *h_distance, mbk_stats *stats);
int mbk_interior_host(double c_r, double c_i, uint32_t mrd, int32_t *count, int32_t *period, int32_t *cycle_len, double *de);
int mbk_view_interior_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                                    const mbk_interior_render_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_view_interior_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags,
                                     const mbk_interior_render_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_interior_resolve_host(const mbk_interior_render_spec *spec, uint32_t width, uint32_t height, const int32_t *counts,
                              const int32_t *period, const double *de, uint8_t *rgba);

/*
 * Relief shading: unit normals of the exterior potential and renders lit from one side.  NOT in the reference; additive (the
 * ABI version stays 5): no existing call changes.  Every colouring above is one scalar per sample through a palette and cannot
 * show slope.  The state of "Distance estimates" holds more than the magnitude 2 |z| ln |z| / |d|: z / d points along the
 * gradient of the exterior potential G(c) = lim 2^-k ln |z_k|, the surface normal of the picture of G as a height field.
 * Lighting the smooth colouring with it makes filaments and spirals stand out as ridges.  For plain views (mbk_view) only.
 *
 * Contract (exact; tests/relief_model.py restates it in numpy, tests/test_relief.py and tests/test_gpu_relief.py hold the host
 * twins and the GPU to it).  Binary64, every operation rounded on its own.
 *   state     exactly that of "Distance estimates": z_0 = c, d_0 = (1, 0), the same step, the same count n, the same run-on (up
 *             to 64 uncounted steps or until mag >= 2^32).
 *   normal    at the final state (zr, zi, dr, di) of a pixel with n > 0: wr = fl(fl(zr dr) + fl(zi di)),
 *             wi = fl(fl(zi dr) - fl(zr di)) -- z conj(d), which has the direction of z / d; m = fl(fl(wr^2) + fl(wi^2)).  If
 *             not m > 0, or m = +inf, the FLAT normal (0, 0) is stored: that covers a NaN, underflow to 0 and overflow.
 *             Otherwise s = fl(sqrt(m)) and (nx, ny) = (fl(wr / s), fl(wi / s)).  Division and square root are the correctly
 *             rounded ones and there is no logarithm, so device, host twin and numpy agree on every bit, the sign of a zero
 *             component included.  n = 0 stores (0, 0).  A NaN is never stored.  mrd 0 and 1 run no step: every normal is
 *             (0, 0).
 *   shade     of a sample under a light (lx, ly) at height h: g = fl(fl(nx lx) + fl(ny ly)), t = fl(fl(g + h) / fl(1 + h));
 *             q = 0 unless t > 0, q = 256 where t >= 1, q = floor(256 t) otherwise (exact).  A flat normal therefore takes the
 *             neutral brightness floor(256 h / (1 + h)).  lx, ly finite with |lx|, |ly| <= 1 (the cosine and sine of an angle,
 *             as a rule, but the contract is on the doubles); h finite with 0 <= h <= 2^10.
 *   colour    of a sample: `inside`, unshaded, if its count is 0.  Otherwise base is the MBK_RENDER_SMOOTH colour of
 *             (count, nu) with the spec's palette, scale and offset (cyclic, 2 <= palette_len <= 65536, the same ranges), and
 *             each of R, G, B becomes (base q + 128) >> 8; alpha is the base's.
 *   rendering resolve, supersampling set (1, 2, 3, 4, 8), output layout, banding under MBK_RENDER_BAND_BYTES, the palette's
 *             wait-on-change rule and the statistics of _compute are those of "Rendering".  Samples are 28 bytes: int32 count,
 *             binary64 nu, two binary64 for the normal.
 * Windows of a view are bit-identical to the whole view; any max_band_rows gives the same image.
 *
 * Held to the mathematics (tests/test_relief.py): the same recurrences with mpmath at 384 bits, from the same binary64 c, give
 * the unit vector of z / d; the model's normal differs from it by 1.4e-15 at c = 0.37 + 0.6i (n = 17), by 3.3e-14 at
 * c = -1.75 + 0.02i (n = 12) and by 6.0e-5 at c = -0.7436438860371587 + 0.1318259043091895i (n = 1194, next to the
 * boundary): rounding in d is amplified exactly as in the distance estimate.
 *
 * Two forms (csrc/mbk_relief.h), those of the distance kernel, storing identical bits: MBK_KERNEL_DEFAULT / _SCAN / _GROUP
 * have the count kernels write the counts (into d_counts, or into scratch the ctx keeps per stream when d_counts is NULL) and
 * run each escaped pixel for exactly its count in a second pass; MBK_KERNEL_ASM carries the derivative in one per-step pass.
 * mbk_view_launch_normal: asynchronous, DEVICE pointers on the caller's stream; d_normal holds two binary64 per pixel of the
 * window, (nx, ny), 8-byte aligned; d_counts and d_distance may be NULL.  d_distance receives the distance estimate of the
 * same final state: the bits mbk_view_launch_distance stores.  Nothing is written outside the window-sized buffers.
 * mbk_view_compute_normal: synchronous into HOST buffers on slot 0 (the slot-0 rule applies), the same pointer rules, stats as
 * for mbk_view_compute_distance.
 * mbk_normal_value_host / mbk_relief_shade_host: the normal of one final state and the shade q of one sample on the HOST,
 * compiled from the functions the kernels use.
 * MBK_ERR_INVALID, with nothing written: whatever mbk_view_launch_distance refuses (MBK_PRECISION_F32, MBK_KERNEL_SIMPLE /
 * _REFILL, mrd >= 2^31, a bad view), any flag bit that is no kernel selector, a NULL normal pointer.
 *
 * Relief renders are calls of their own, not an MBK_RENDER_* source.  A band computes the samples of mbk_view_launch_smooth
 * (counts and nu, with the kernel `flags` select), runs the two-pass normal kernel on those counts and resolves.
 * MBK_ERR_INVALID, with nothing written: whatever mbk_view_render_* refuses for MBK_RENDER_SMOOTH, a NULL spec, palette or
 * output pointer, a light or a height that is not finite or lies outside its range.
 * mbk_relief_resolve_host: colour and resolve on the HOST for caller-supplied samples of (width s) x (height s); `normals`
 * holds two binary64 per sample.
 *
 * Out of scope: Julia views (deep and extended-range deep views: the two sections below); adaptive supersampling; equalised or
 * distance base colours; sharding and slot forms; specular terms.
 */
typedef struct mbk_relief_spec {
    uint32_t supersample;   /* 1, 2, 3, 4, 8 */
    const uint8_t *palette; /* HOST pointer, palette_len x RGBA8; copied during the call */
    uint32_t palette_len;   /* 2 .. 65536 */
    uint8_t inside[4];      /* the colour of a sample that never escapes; not shaded */
    double scale, offset;   /* as for MBK_RENDER_SMOOTH */
    double light_x, light_y; /* the light's direction in the plane, each in [-1, 1] */
    double height;          /* the light's height above the plane, 0 .. 2^10 */
    uint32_t max_band_rows; /* 0 = the library's choice; any value gives the same image */
} mbk_relief_spec;
int mbk_view_launch_normal(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *d_counts,
                           double *d_normal, double *d_distance, void *hip_stream);
int mbk_view_compute_normal(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, int32_t *h_counts,
                            double *h_normal, double *h_distance, mbk_stats *stats);
int mbk_normal_value_host(double zr, double zi, double dr, double di, int32_t count, double out[2]);
uint32_t mbk_relief_shade_host(double nx, double ny, double lx, double ly, double h);
int mbk_view_relief_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_relief_spec *spec,
                                  uint8_t *d_rgba, void *hip_stream);
int mbk_view_relief_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_relief_spec *spec,
                                   uint8_t *h_rgba, mbk_stats *stats);
int mbk_relief_resolve_host(const mbk_relief_spec *spec, uint32_t width, uint32_t height, const int32_t *counts,
                            const double *smooth, const double *normals, uint8_t *rgba);

/*
 * Stripe-average colouring: a statistic taken along a pixel's own orbit, and renders shaded by it.  NOT in the reference;
 * additive (the ABI version stays 5): no existing call changes.  Every colouring above is a function of a pixel's final state;
 * the stripe average (Harkonen) is the mean of 1/2 + 1/2 sin(s arg z_k) over the orbit, interpolated across the escape bands so
 * that the picture is continuous -- the striped, feathered exteriors of Mandelbrot renderers.  For an integer density s,
 * sin(s arg z) is the imaginary part of (z / |z|)^s: one square root, two divisions and s - 1 complex products, all correctly
 * rounded, no libm call per step.  For plain views (mbk_view) only.
 *
 * Contract (exact; tests/stripe_model.py restates it in numpy, tests/test_stripe.py and tests/test_gpu_stripe.py hold the host
 * twins and the GPU to it).  Binary64, every operation rounded on its own.  Uniform per launch: the density s in 1 .. 16 and
 * skip in 0 .. 2^31 - 1, the number of leading orbit points left out of the average.
 *   orbit     z_0 = c, the recurrence and the count n of mbk_view_launch, unchanged.  The run-on is that of "Distance estimates":
 *             a pixel with n > 0 runs on, uncounted, until mag = fl(fl(zr^2) + fl(zi^2)) >= 2^32 or 64 further steps.
 *             N = n + run-on steps is the index of the last point.
 *   term      of a point z_k, 1 <= k <= N: if not mag_k > 0, or mag_k = +inf, t_k = 0.5 (that covers NaN and 0).  Otherwise
 *             r = fl(sqrt(mag_k)), u = (fl(zr / r), fl(zi / r)), p = u, then s - 1 times
 *             p <- (fl(fl(p.r u.r) - fl(p.i u.i)), fl(fl(p.r u.i) + fl(p.i u.r))), and t_k = fl(0.5 + fl(0.5 p.i)).
 *   sum       S adds t_k for k = skip + 1 .. N in ascending order, one rounded addition each; cnt = max(0, N - skip);
 *             t_last = t_N if cnt > 0, else 0.  The exact state of a pixel is (n, N, S, t_last, mag_N, cnt); a pixel with
 *             n = 0 has the all-zero state.
 *   value     v = 0 if n = 0; 0.5 if cnt = 0; S if cnt = 1.  Otherwise a1 = fl(S / cnt), a0 = fl(fl(S - t_last) / (cnt - 1)),
 *             d = fl(1 - fl(log2(fl(fl(ln mag_N) / LB)))) with LB the binary64 nearest 32 ln 2; d = 0 unless d >= 0 (a NaN,
 *             mag = inf), d = 1 where d > 1 (the 64-step cap: c = -2); v = fl(a0 + fl(fl(a1 - a0) d)).  a0 comes from
 *             S - t_last, not from a second running sum.  ln and log2 are the device's (ocml) on the device and the C
 *             library's on the host; everything else is exact.  A NaN is never stored.
 *   shade     of a sample, lo in [0, 1] and gain finite in [0, 2^10]: w = fl(0.5 + fl(gain fl(v - 0.5))) clamped to [0, 1],
 *             t = fl(lo + fl(fl(1 - lo) w)), q = floor(256 t), or 256 where t >= 1.
 *   colour    of a sample: `inside`, unshaded, if its count is 0.  Otherwise base is the MBK_RENDER_SMOOTH colour of
 *             (count, nu) with the spec's palette, scale and offset, and each of R, G, B becomes (base q + 128) >> 8, exactly
 *             as the relief rule scales; alpha is the base's.
 *   rendering resolve, supersampling set, output layout, banding, the palette's wait-on-change rule and the statistics of
 *             _compute are those of "Rendering".  Samples are 20 bytes: int32 count, binary64 nu, binary64 v.
 * mrd 0 and 1 run no step: every count and value is 0.  Windows of a view are bit-identical to the whole view; any
 * max_band_rows gives the same image.
 *
 * Held to the mathematics (tests/test_stripe.py): the same recurrences and the true sin(s arg z_k) with mpmath at 384 bits, from
 * the same binary64 c, against the model's v at s = 1, 5, 16 (tests/stripe_model.py: MEASURED_TRUTH): 2.2e-16 .. 2.5e-15 at
 * c = 0.37 + 0.6i (n = 17), 1.9e-14 .. 1.6e-13 at c = -1.75 + 0.02i (n = 12), 7.6e-7 .. 6.2e-6 at
 * c = -0.7436438860371587 + 0.1318259043091895i (n = 1194, next to the boundary, where rounding in z is amplified as it is
 * for the normals).  The value expression is within 1.45 ulp(v) of its correctly rounded value on the host
 * (MEASURED_VALUE_ULPS_HOST, over the escaped pixels of a 67 x 45 view of the seahorse valley), one ulp more on the device.
 * Along ci = 0.6 near cr = 0.404631, where N changes, the largest difference between neighbouring samples at density 5 halves
 * with the spacing (3.0e-3 at 1e-9): steep, not a jump.
 *
 * One form (csrc/mbk_stripe.h), the two-pass form of the distance kernel: MBK_KERNEL_DEFAULT / _SCAN / _GROUP have the count
 * kernels write the counts (into d_counts, or into scratch the ctx keeps per stream when d_counts is NULL), and a second
 * kernel replays each escaped pixel for exactly its count and then the run-on.
 * mbk_view_launch_stripe: asynchronous, DEVICE pointers on the caller's stream; d_stripe holds one binary64 per pixel of the
 * window, 8-byte aligned; d_counts and d_state may be NULL.  d_state receives the exact state, 32 bytes per pixel in five
 * arrays of px = ncols * nrows elements each, one after the other: S, t_last and mag_N as binary64, then N and cnt as int32;
 * 8-byte aligned.  Nothing is written outside the window-sized buffers.  The launch forms obey "Graph capture" and "Streams".
 * mbk_view_compute_stripe: synchronous into HOST buffers on slot 0 (the slot-0 rule applies), the same pointer rules and the
 * same state layout, stats as for mbk_view_compute_distance.
 * mbk_stripe_state_host: one pixel by coordinate on the HOST (the literal doubling throughout); mbk_stripe_value_host /
 * mbk_stripe_shade_host: the value of one exact state and the shade q of one sample, compiled from the functions the kernel uses.
 * MBK_ERR_INVALID, with nothing written: whatever mbk_view_launch_distance refuses (MBK_PRECISION_F32, MBK_KERNEL_SIMPLE /
 * _REFILL, mrd >= 2^31, a bad view), MBK_KERNEL_ASM (there is no one-pass form), any flag bit that is no kernel selector, a
 * density outside 1 .. 16, a skip above 2^31 - 1, a NULL value pointer.
 *
 * Stripe renders are calls of their own, not an MBK_RENDER_* source.  A band computes the samples of mbk_view_launch_smooth
 * (counts and nu, with the kernel `flags` select), runs the stripe kernel on those counts and resolves.
 * MBK_ERR_INVALID, with nothing written: whatever mbk_view_render_* refuses for MBK_RENDER_SMOOTH, a NULL spec, palette or
 * output pointer, a density or skip out of range, a lo or gain that is not finite or lies outside its range.
 * mbk_stripe_resolve_host: colour and resolve on the HOST for caller-supplied samples of (width s) x (height s).
 *
 * Out of scope: Julia, deep and extended-range views; adaptive supersampling, sharding and slot forms; a one-pass or fp32
 * form; other orbit statistics (triangle-inequality average, orbit traps); combining stripes with relief.
 */
typedef struct mbk_stripe_state {
    double S, t_last, mag; /* the sum, the last term, mag_N */
    double v;              /* the value of this state */
    int32_t n, N, cnt;     /* the count, the index of the last point, the number of terms in S */
    int32_t reserved;      /* 0 */
} mbk_stripe_state;
typedef struct mbk_stripe_spec {
    uint32_t supersample;   /* 1, 2, 3, 4, 8 */
    const uint8_t *palette; /* HOST pointer, palette_len x RGBA8; copied during the call */
    uint32_t palette_len;   /* 2 .. 65536 */
    uint8_t inside[4];      /* the colour of a sample that never escapes; not shaded */
    double scale, offset;   /* as for MBK_RENDER_SMOOTH */
    uint32_t density;       /* s, 1 .. 16 */
    uint32_t skip;          /* leading orbit points left out, 0 .. 2^31 - 1 */
    double lo;              /* the brightness of the darkest stripe, 0 .. 1 */
    double gain;            /* contrast about v = 0.5, 0 .. 2^10 */
    uint32_t max_band_rows; /* 0 = the library's choice; any value gives the same image */
} mbk_stripe_spec;
int mbk_view_launch_stripe(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t density, uint32_t skip,
                           int32_t *d_counts, double *d_stripe, void *d_state, void *hip_stream);
int mbk_view_compute_stripe(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t density, uint32_t skip,
                            int32_t *h_counts, double *h_stripe, void *h_state, mbk_stats *stats);
int mbk_stripe_state_host(double c_r, double c_i, uint32_t mrd, uint32_t density, uint32_t skip, mbk_stripe_state *out);
double mbk_stripe_value_host(double S, double t_last, int32_t cnt, double mag, int32_t count);
uint32_t mbk_stripe_shade_host(double v, double lo, double gain);
int mbk_view_stripe_render_launch(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_stripe_spec *spec,
                                  uint8_t *d_rgba, void *hip_stream);
int mbk_view_stripe_render_compute(mbk_ctx *ctx, const mbk_view *view, uint32_t mrd, uint32_t flags, const mbk_stripe_spec *spec,
                                   uint8_t *h_rgba, mbk_stats *stats);
int mbk_stripe_resolve_host(const mbk_stripe_spec *spec, uint32_t width, uint32_t height, const int32_t *counts,
                            const double *smooth, const double *stripe, uint8_t *rgba);

/*
 * Relief shading for deep views: the same normals and lit renders for mbk_deep_view, with the plain step and with the skips of
 * MBK_DEEP_BLA.  NOT in the reference; additive (the ABI version stays 5): no existing call changes.  At a span of 1e-60 a
 * count or nu picture is dense bands; slope lighting is what makes filaments and spirals readable there, and it is nearly free:
 * the deep distance kernels already end every escaped pixel with its full z and the derivative D 2^e in registers.
 *
 * Contract (exact; tests/deep_relief_model.py restates it in numpy, tests/test_deep_relief.py and tests/test_gpu_deep_relief.py
 * hold the host twin and the GPU to it).  Binary64, every operation rounded on its own.
 *   state     flags 0: exactly that of "Distance estimates for deep views"; flags MBK_DEEP_BLA: exactly that of "Distance
 *             estimates for deep views with bilinear approximation" -- the same start, step (and skip), rescale rule, count n,
 *             run-on and final (zp, D, e), zp being the pixel's full z = fl(Z_m + dz) of the last step run.
 *   normal    normal_value(zp.r, zp.i, D_r, D_i, n) as "Relief shading" defines it on (z, d): the same products, the same
 *             flat-normal rule, the correctly rounded square root and division.  e is NOT used: the direction of z conj(d)
 *             does not depend on the scale of d, so D stands for d = D 2^e and a view at e = 768 needs nothing more than one
 *             at e = 0.  m = |zp conj(D)|^2 cannot overflow: the rescale rules leave max(|D_r|, |D_i|) < 2^256 and the run-on
 *             stops at the first |zp|^2 >= 2^32, reached from below 2^32, so |zp|^2 < 2^65 and m < 2^(65 + 514) < 2^580.
 *             m CAN underflow to 0, and the normal of an escaped pixel is then flat; |zp| >= 2 there, so it needs
 *             max(|D_r|, |D_i|) < 2^-538, and nothing in the rules forbids that.  The plain step rescales downwards only: a step
 *             from |zp| < 1/2 shrinks D and e does not fall.  The skip's upward rescale is applied once per skip, by 2^256,
 *             and only while e >= 256: it brings max(|D_r|, |D_i|) back to 2^-256 or above only from 2^-512 or above.  With
 *             e < 256 such a D is a true |d| < 2^-282 -- the pixel sits on a critical point of z_n(c), where the gradient has
 *             no direction and rel is +inf or overflows; with e >= 256 it takes 282 binades of decay after the last restoring
 *             skip.  Neither occurs on the project's cases (the tests assert that every escaped pixel's normal is a unit
 *             vector); where it does, (0, 0) is the defined result.
 *   nu        smooth_value(n, mag) with the mag of the ESCAPING step, before the run-on: the bits mbk_deep_view_launch stores
 *             as smooth values under the same flags.
 *   rel       (optional output) the bits mbk_deep_view_launch_distance stores; with MBK_DEEP_BLA those of
 *             mbk_deep_view_launch_distance_bla.
 *   shade, colour, resolve, banding, statistics: those of "Relief shading" and "Rendering".  A sample is 28 bytes.
 *             mbk_relief_spec and mbk_relief_resolve_host serve as they are.
 * Windows of a view are bit-identical to the whole view (the table of MBK_DEEP_BLA is the FULL view's); any max_band_rows
 * gives the same image.  mrd 0 and 1 run no step: every count and nu is 0 and every normal flat.  Where no skip is ever taken
 * (M <= 1, or offsets that never pass the radius test) MBK_DEEP_BLA changes no bit.
 * Held to the mathematics (tests/test_deep_relief.py): d' = 2 z d + 1, z' = z^2 + c in mpmath at the orbit's precision + 128
 * bits from the exact pixel coordinate give the unit vector of z / d; the model's normal is within 4 x MEASURED_NORMAL of it
 * (tests/deep_relief_model.py, measured per case with and without skips) on the escaped picks whose count and run-on agree.
 *
 * ONE pass (csrc/mbk_deep_relief.h): the loops of the deep distance kernels with another epilogue; a deep sample costs
 * thousands of perturbation steps and is paid once, whatever is asked for.  With M <= 1 the flag changes nothing.
 * mbk_deep_view_launch_normal: asynchronous, DEVICE pointers on the caller's stream.  d_normal: two binary64 per pixel of the
 * window, 8-byte aligned, required; d_counts (int32), d_smooth (nu) and d_rel (binary64 each) may be NULL.  Nothing is written
 * outside the window-sized buffers.  flags: 0 or MBK_DEEP_BLA -- the calls are new, so the flag is taken on the one name.  The
 * table is the one the MBK_DEEP_BLA count launches build and share, under their first-launch rule: launch once per (orbit,
 * spans) before capturing.
 * mbk_deep_view_compute_normal: synchronous into HOST buffers on slot 0 (the slot-0 rule applies), the same pointer rules;
 * pixel_iterations counts the reference's iterations (count, or mrd - 1 for 0), not the steps executed and not the run-on.
 * mbk_deep_view_relief_render_launch / _compute: a band runs the one-pass kernel for counts, nu and normals and resolves with
 * the relief rule.
 * mbk_deep_normal_host: one pixel (col, row) of the FULL view on the HOST, compiled from the functions the kernels use: count,
 * run-on steps, final zp, D and e, the normal, nu, and the steps executed in the count loop (a skip is one).
 * MBK_ERR_INVALID, with nothing written: whatever mbk_deep_view_launch_distance refuses for the view, the orbit and mrd (with
 * MBK_DEEP_BLA also an orbit longer than 2^31); any flag bit other than MBK_DEEP_BLA; ranges below 2^-960 (an extended-range
 * view has no call here); a NULL normal, spec, palette or output pointer; a light or a height outside the ranges of "Relief
 * shading".
 *
 * Out of scope: Julia views (extended-range views: "Relief shading for extended-range deep views", below); adaptive
 * supersampling; sharding and slot forms.
 */
int mbk_deep_view_launch_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                uint32_t flags, int32_t *d_counts, double *d_normal, double *d_smooth, double *d_rel,
                                void *hip_stream);
int mbk_deep_view_compute_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                 uint32_t flags, int32_t *h_counts, double *h_normal, double *h_smooth, double *h_rel,
                                 mbk_stats *stats);
int mbk_deep_view_relief_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                       uint32_t flags, const mbk_relief_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_deep_view_relief_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t mrd,
                                        uint32_t flags, const mbk_relief_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_deep_normal_host(const mbk_deep_orbit *orbit, const mbk_deep_view *view, uint32_t col, uint32_t row, uint32_t mrd,
                         uint32_t flags, int32_t *count, int32_t *extra, double *zp_r, double *zp_i, double *D_r, double *D_i,
                         int32_t *e, double normal[2], double *nu, uint64_t *steps_executed);

/*
 * Relief shading for extended-range deep views: the same normals and lit renders for mbk_deep_xview (spans below 2^-960), with
 * the plain wide step and with the skips of MBK_DEEP_XBLA.  NOT in the reference; additive (the ABI version stays 5): no
 * existing call changes.  Past 2^-960 a count or nu picture is dense bands and slope lighting is what keeps filaments
 * readable; it is nearly free, since the wide distance kernels already end every escaped pixel with its full z = (zr, zi) 2^t
 * and the derivative d = (Dr, Di) 2^e in registers.
 *
 * Contract (exact; tests/deep_wide_relief_model.py restates it in numpy, tests/test_deep_wide_relief.py and
 * tests/test_gpu_deep_wide_relief.py hold the host twin and the GPU to it).  Binary64 mantissas, every operation rounded on its
 * own.
 *   state     flags 0: exactly that of "Distance estimates for extended-range deep views"; flags MBK_DEEP_XBLA: exactly that
 *             of "Distance estimates for extended-range deep views with bilinear approximation" -- the same start, step (and
 *             skip), count n, run-on and final (zr, zi, t, Dr, Di, e): zp = (zr, zi) 2^t is step (e)'s sum of the last step
 *             run, on its nominal exponent, not renormalised.
 *   normal    normal_value(zr, zi, Dr, Di, n) as "Relief shading" defines it on (z, d): the same products, the same
 *             flat-normal rule, the correctly rounded square root and division.  Neither t nor e is used: the direction of
 *             z conj(d) depends on the scale of neither factor.
 *   bound     m = |(zr, zi) conj((Dr, Di))|^2 of an escaped pixel with D != 0 lies in (2^-68, 2^5): it can neither overflow
 *             nor underflow.  Above: zr and zi are each the sum of two aligned mantissas below 1 in magnitude, so
 *             |zr|, |zi| < 2; max(|Dr|, |Di|) < 1; each of the two sums of products is below 4 and m < 32.  Below: the
 *             escaping |z|^2 >= 4 as computed, so |z| >= 2 (1 - 2^-50), and |z| does not shrink in the run-on, which stops
 *             at the first |z|^2 >= 2^32, reached from below 2^32 with |c| < 3: |z| < 2^32 + 3.  The orbit ends at its first
 *             |Z_M|^2 >= 4, so |Z_m| < 6 and its exponent xe <= 3; |dz| <= |z| + |Z_m| < 2^33 gives q <= 33.  t = max(xe, q)
 *             <= 33, so |(zr, zi)|^2 = |z|^2 2^(-2t) > 2^-65; the larger component of D is at least 1/2, |D|^2 >= 1/4; the
 *             roundings of the four products, two sums, two squares and the last sum move m by a relative 2^-49 at most
 *             (one of the two sums of products may cancel; the other then carries m).  So the flat normal of an escaped pixel
 *             means D == 0 exactly -- 2 z d = -1 to the last bit at the step before, the critical point where the gradient
 *             has no direction -- and the 2^-538 caveat of "Relief shading for deep views" has no counterpart.  The tests
 *             assert that no escaped pixel of any case is flat.
 *   nu        smooth_value(n, mag) with the mag of the ESCAPING step, before the run-on: the bits mbk_deep_xview_launch
 *             stores as smooth values under the same flags.
 *   rel       (optional output) the bits mbk_deep_xview_launch_distance stores; with MBK_DEEP_XBLA those of
 *             mbk_deep_xview_launch_distance_xbla.
 *   shade, colour, resolve, banding, statistics: those of "Relief shading" and "Rendering".  A sample is 28 bytes.
 *             mbk_relief_spec and mbk_relief_resolve_host serve as they are.
 * Wherever the plain deep contract meets no subnormal, the normal is the one "Relief shading for deep views" stores, bit for
 * bit (scaling by a power of two is exact).  Windows of a view are bit-identical to the whole view (the table of MBK_DEEP_XBLA
 * is the FULL view's; for a render at supersample s, the sample view's own); any max_band_rows gives the same image.  mrd 0
 * and 1 run no step: every count and nu is 0 and every normal flat.  Where no skip is ever
 * taken (M <= 1, or offsets that never pass the radius test) MBK_DEEP_XBLA changes no bit.
 * Held to the mathematics (tests/test_deep_wide_relief.py): d' = 2 z d + 1, z' = z^2 + c in mpmath at the orbit's precision +
 * 128 bits from the exact pixel coordinate give the unit vector of z / d; the model's normal is within 4 x MEASURED_NORMAL of
 * it (tests/deep_wide_relief_model.py, measured per case with and without skips) on the escaped picks whose count and run-on
 * agree.
 *
 * ONE pass (csrc/mbk_deep_wide_relief.h): the loops of the wide distance kernels with another epilogue; a wide sample costs
 * thousands of wide steps and is paid once, whatever is asked for.
 * mbk_deep_xview_launch_normal: asynchronous, DEVICE pointers on the caller's stream.  d_normal: two binary64 per pixel of the
 * window, 8-byte aligned, required; d_counts (int32), d_smooth (nu) and d_rel (binary64 each) may be NULL.  Nothing is written
 * outside the window-sized buffers.  flags: 0 or MBK_DEEP_XBLA.  The table is the one the MBK_DEEP_XBLA count launches build
 * and share (two per orbit), under their first-launch rule: launch once per (orbit, spans) before capturing.
 * mbk_deep_xview_compute_normal: synchronous into HOST buffers on slot 0 (the slot-0 rule applies), the same pointer rules.
 * mbk_deep_xview_relief_render_launch / _compute: a band runs the one-pass kernel for counts, nu and normals and resolves
 * with the relief rule.
 * mbk_deep_xview_normal_host: one pixel (col, row) of the FULL view on the HOST, compiled from the functions the kernels use:
 * count, run-on steps, final zp = (zp_r, zp_i) 2^zp_t, D and e, the normal, nu (through the host's logarithms), and the steps
 * executed in the count loop (a skip is one).  No ctx, no device.
 * MBK_ERR_INVALID, with nothing written: whatever mbk_deep_xview_launch refuses for the view, the orbit and mrd under the same
 * flags; MBK_DEEP_BLA, in the count calls' words; any other flag bit than MBK_DEEP_XBLA; a NULL normal, spec, palette or
 * output pointer; a misaligned d_normal or d_rgba; a light or a height outside the ranges of "Relief shading".
 *
 * Out of scope: adaptive supersampling of relief renders; Julia views; stored chunks; sharding and slot forms.
 */
int mbk_deep_xview_launch_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                 uint32_t flags, int32_t *d_counts, double *d_normal, double *d_smooth, double *d_rel,
                                 void *hip_stream);
int mbk_deep_xview_compute_normal(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                  uint32_t flags, int32_t *h_counts, double *h_normal, double *h_smooth, double *h_rel,
                                  mbk_stats *stats);
int mbk_deep_xview_relief_render_launch(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                        uint32_t flags, const mbk_relief_spec *spec, uint8_t *d_rgba, void *hip_stream);
int mbk_deep_xview_relief_render_compute(mbk_ctx *ctx, const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t mrd,
                                         uint32_t flags, const mbk_relief_spec *spec, uint8_t *h_rgba, mbk_stats *stats);
int mbk_deep_xview_normal_host(const mbk_deep_orbit *orbit, const mbk_deep_xview *view, uint32_t col, uint32_t row,
                               uint32_t mrd, uint32_t flags, int32_t *count, int32_t *extra, double *zp_r, double *zp_i,
                               int32_t *zp_t, double *D_r, double *D_i, int32_t *e, double normal[2], double *nu,
                               uint64_t *steps_executed);

/* Codec codes of DataChunkSerializer.cs (Raw :20, RLE :54). */
#define MBK_CODEC_RAW 0x00u
#define MBK_CODEC_RLE 0x01u

/* Serialise, ON THE DEVICE, the quantised bytes of the last tile this ctx computed with
 * MBK_WANT_BYTES (mbk_datachunk / mbk_view_compute): exactly the byte stream DataChunk.Serialize
 * (DataChunk.cs:173-206) writes to a chunk file / the DataServer sends to the Viewer
 * (DataServer.cs:204-220): one code byte, then the Raw payload (the n bytes) or the RLE payload
 * (repeated u32 runLength LE + u8 value, DataChunkSerializer.cs:56-100), whichever is strictly
 * shorter, Raw winning ties (serializer order, DataChunk.cs:165-168,190).  Only the serialised bytes
 * cross PCIe.  h_out must hold *size <= 1 + n bytes; cap is its capacity (MBK_ERR_INVALID if too
 * small, with *size set to the needed size). */
int mbk_serialize_last(mbk_ctx *ctx, uint8_t *h_out, uint64_t cap, uint64_t *size, uint32_t *codec);

/*
 * Stored chunks: the inverse of mbk_serialize_last, and the picture of a chunk.  A chunk that lies in a store or comes from a
 * DataServer is decoded ON THE DEVICE, coloured through a 256-entry palette and box-filtered into an RGBA8 rectangle that may
 * lie inside a larger image -- what the reference's Viewer does on the host for one chunk at full size
 * (DistributedMandelbrotViewer.py:35-60,110-135).  Additive (the ABI version stays 5): no existing call changes.
 *
 * Contract (bit-exact; tests/chunk_model.py restates it in numpy, tests/test_chunks.py and tests/test_gpu_chunks.py hold the
 * host and the GPU to it):
 *   stream    what DataChunk.Serialize writes (DataChunk.cs:173-206): one code byte, then a payload, `size` bytes in all, for a
 *             chunk of n bytes, 1 <= n <= MBK_CHUNK_BYTES (the render calls take n = MBK_CHUNK_BYTES only).
 *             MBK_CODEC_RAW: valid iff size >= 1 + n; the chunk is the first n payload bytes, what follows is ignored.
 *             MBK_CODEC_RLE: records of 5 bytes (u32 run length, little-endian; u8 value).  Valid iff the payload length is a
 *             multiple of 5, size <= 1 + n, no run length is 0 and the run lengths sum to exactly n, the sum taken in 64 bits
 *             (lengths are arbitrary u32: a sum that wraps does not pass).  Runs need not be maximal: equal neighbouring
 *             values are legal.  Against the reference's reader (DataChunkSerializer.cs:102-142) this is stricter in one
 *             respect: the C# loop stops reading once n bytes are filled and never looks at trailing records, which are
 *             refused here.  The limit size <= 1 + n bounds the scratch (an accepted stream holds at most n / 5 runs); no
 *             serializer writes a longer RLE stream (Raw wins unless RLE is strictly shorter, DataChunk.cs:186-196).
 *             Any other code is invalid.
 *   reason    why a stream is invalid, MBK_STREAM_*.  Where several apply, the first of this list wins, on the host and on
 *             the device alike: _BAD_SIZE for an empty stream (size 0: there is no code byte); _BAD_CODEC; _BAD_SIZE (Raw
 *             shorter than 1 + n; RLE payload not a multiple of 5; RLE longer than 1 + n); _ZERO_RUN (a zero run anywhere,
 *             whatever the sum); _TOO_LONG (sum > n); _TOO_SHORT (sum < n; an RLE stream of the code byte alone is that).
 *   colour    a chunk rendered at scale k in {1, 2, 4, 8, 16, 32, 64}: output pixel (x, y) owns the bytes of columns
 *             x k .. x k + k - 1 and rows y k .. y k + k - 1 of the 4096 x 4096 chunk; its colour is, per channel, alpha
 *             included, (2 S + k^2) / (2 k^2) rounded down, S the sum of palette[b] over its k^2 bytes -- "resolve" of the
 *             Rendering section with 32-bit sums.  The palette is 256 RGBA8 entries (HOST pointer, copied during the call, as
 *             for MBK_RENDER_BYTES).  A chunk of one value v therefore renders as palette[v] exactly, at every k.
 *   output    (4096 / k) rows of (4096 / k) pixels, row 0 the lowest imaginary part; pixel (x, y) at byte 4 (y pitch_px + x),
 *             pitch_px >= 4096 / k, so that a chunk can land inside a larger image.  Nothing between the rows is written.
 *
 * The host forms need no ctx and no device; they are the functions the kernels are compiled from.  _launch: asynchronous on
 * the caller's HIP stream.  h_stream is a HOST pointer that must stay valid until the stream has passed the copy (pinned
 * memory, mbk_host_alloc, makes the copy asynchronous).  What the host sees without walking the payload -- NULL pointers, n or
 * scale out of range, the code byte, the size rules, and a stream of a single record -- is refused at once with
 * MBK_ERR_INVALID, nothing enqueued, d_status untouched.  Run lengths are validated ON THE DEVICE (the prefix sum that the
 * expansion needs yields the total; the zero-run test is a reduction) and the reason code is written to d_status (a device
 * uint32_t, may be NULL; MBK_STREAM_OK for a valid stream).  Whatever the stream holds, nothing is written outside the n
 * output bytes / the (4096 / k)^2 output pixels: after a non-zero status the contents of the output are unspecified, its bounds
 * are not.  d_rgba must be 4-byte aligned.  A stream of one run (what a DataServer sends for a Never / Immediate chunk) is not
 * expanded: the output is filled with the value / with palette[value], bit-identical to the long way round.
 * _compute: synchronous on slot 0 (the slot-0 rule applies); an invalid stream returns MBK_ERR_INVALID (mbk_last_error names
 * the reason) with the host buffer untouched.  stats: kernel_ms (from the end of the stream's upload to the end of the decode /
 * resolve kernels: next to nothing for the decode of a Raw stream, which IS its upload), d2h_ms; for decode also
 * all_bytes_zero, all_bytes_one and rle_runs of the DECODED chunk (maximal runs, so a caller can re-derive the codec choice);
 * the other fields 0.  mbk_serialize_last is not affected: it still refers to the last tile computed with bytes.
 *
 * Memory: per stream, grown on demand, freed with the ctx: the uploaded payload (<= 16 MiB), the run starts and values
 * (5 bytes x n / 5), the decoded bytes of the render form (16 MiB), the palette (shared with the renders of that stream; the
 * same wait-on-change rule).  mbk_chunk_render_compute uses the ctx's device image of the synchronous renders.
 *
 * Out of scope: overlapping one chunk's upload with another's kernels (slot / submit forms), and mosaics in native code
 * (distributedmandelbrot_amd/viewer.py places chunks through pitch_px).
 */
#define MBK_STREAM_OK 0u
#define MBK_STREAM_BAD_CODEC 1u
#define MBK_STREAM_BAD_SIZE 2u
#define MBK_STREAM_ZERO_RUN 3u
#define MBK_STREAM_TOO_LONG 4u
#define MBK_STREAM_TOO_SHORT 5u

typedef struct mbk_chunk_spec {
    const uint8_t *palette; /* HOST pointer, 256 x RGBA8; copied during the call */
    uint32_t scale;         /* k: 1, 2, 4, 8, 16, 32, 64 */
} mbk_chunk_spec;

/* MBK_OK, or MBK_ERR_INVALID with *reason set (MBK_STREAM_BAD_SIZE also for n outside [1, MBK_CHUNK_BYTES]).  *codec: the code
 * byte; *runs: the records of an RLE payload, 0 for Raw.  Any output pointer may be NULL. */
int mbk_chunk_stream_check(const uint8_t *stream, uint64_t size, uint64_t n, uint32_t *codec, uint64_t *runs, uint32_t *reason);
/* The decoded chunk into bytes[n], or MBK_ERR_INVALID with nothing written. */
int mbk_chunk_decode_host(const uint8_t *stream, uint64_t size, uint64_t n, uint8_t *bytes);
/* "colour" and "output" above for a decoded 4096 x 4096 chunk. */
int mbk_chunk_resolve_host(const mbk_chunk_spec *spec, const uint8_t *bytes, uint8_t *rgba, uint64_t pitch_px);
int mbk_chunk_decode_launch(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, uint64_t n, uint8_t *d_bytes,
                            uint32_t *d_status, void *hip_stream);
int mbk_chunk_render_launch(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, const mbk_chunk_spec *spec, uint8_t *d_rgba,
                            uint64_t pitch_px, uint32_t *d_status, void *hip_stream);
int mbk_chunk_decode_compute(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, uint64_t n, uint8_t *h_bytes,
                             mbk_stats *stats);
int mbk_chunk_render_compute(mbk_ctx *ctx, const uint8_t *h_stream, uint64_t size, const mbk_chunk_spec *spec, uint8_t *h_rgba,
                             uint64_t pitch_px, mbk_stats *stats);

/*
 * Tuning options.  They change scheduling only -- every value the setter accepts gives bit-identical
 * results (tests/test_gpu_parity.py::test_option_matrix_is_bit_exact) -- and the library reads NO
 * environment variable.  mbk_set_option returns MBK_ERR_INVALID for an unknown option or a value out of
 * range.  Defaults in brackets.
 */
enum mbk_option {
    MBK_OPT_ORDER = 0,     /* asm/group: workgroup order ([3] since round 4). 0 image order, 1 multiplicative permutation, 2 heavy-first list
                              (probe never escaped first; optionally a middle class, MBK_OPT_PROBE_MID), 3 "units" (round 4,
                              csrc/mbk_units.h): probe never escaped / escaped at step 4..31 one workgroup per block in that
                              order, then the blocks whose probe escaped within 3 steps eight block columns to a workgroup
                              through the light path; launches it has no form for (kernel "asm", smooth output, 64-bit
                              quantiser, block columns not a multiple of 8 or > 2048, group_steps != 16) take order 2 */
    MBK_OPT_WAVES_PER_WG,  /* asm/group: 8x8 blocks per workgroup: [1], 2, 4 */
    MBK_OPT_GROUP_STEPS,   /* group: steps per grouped bailout test: 4, 8, [16], 32 (16 / 32 apply to the blocks classified as
                              interior -- probe-heavy / dense --, the rest keep 8).  Scan pass 2 and the fp32 loops have no
                              4-step form: there 4 means 8 (and the cycle test needs >= 8, so 4 in "group" runs without it).
                              32 exists for the fp64 "group" kernel without the cycle test only; everywhere else it means 16 */
    MBK_OPT_EXACT_STEPS,   /* group / scan pass 2: steps tested one by one before the grouped test takes over: 0..4096 [8] */
    MBK_OPT_PROBE_STEPS,   /* asm/group: depth of the heavy-first probe: 2..65536 [32] */
    MBK_OPT_SCAN_WAVES,    /* scan: resident waves per SIMD of pass 1: 1..[8] */
    MBK_OPT_SCAN_XCD_MAP,  /* scan: XCD-aware block-column order (a 128-byte output line is completed in one L2): 0, [1] */
    MBK_OPT_SCAN_COL_PERIOD, /* scan: sweeps a pass-1 wave stays in one block column before jumping to a far one: 0 (never) .. 65536 [4] */
    MBK_OPT_HEAVY_SHARE,   /* default kernel: share (x 65536) of the window's probe pixels still inside after 4 steps above
                              which the launch uses "group" instead of "scan": 0 (always group) .. 65536 (always scan) [655 = 1 %] */
    MBK_OPT_RF_LIVEMIN,    /* refill: refill when this many lanes or fewer are live: 0..63 [48] */
    MBK_OPT_RF_PATIENCE,   /* refill: steps between forced refill checks: 16..2^20 [256] */
    MBK_OPT_RF_BATCH,      /* refill: blocks per queue pop: 1..64 [1] */
    MBK_OPT_RF_WAVES,      /* refill: resident waves per SIMD: 1..[8] */
    MBK_OPT_CYCLE_DETECT,  /* group / scan pass 2 (8- and 16-step groups): retire a pixel as "never escapes" as soon as its
                              (zr, zi) bit pattern repeats an earlier state of its own orbit -- the step map is a
                              deterministic function of those bits, so the reference's loop provably runs to mrd-1 and
                              returns 0.  Same counts, fewer executed steps on tiles that hold part of the set: 0, [1] */
    MBK_OPT_PROBE_MID,     /* asm/group: a block whose probe pixel escapes at step >= this value goes to a middle dispatch
                              class (after the blocks whose probe never escaped, before the rest): 2..[65537]; a value
                              above probe_steps leaves the middle class empty = the two-class order.  Measured on cfg2
                              (profiles/r03): 6 -> 581.8 us per launch, off -> 577.8: the light blocks are dispatch-bound
                              and must stay interleaved with the boundary blocks, so the default is off */
    MBK_OPT_PREPASS_OVERLAP, /* asm/group: run the dispatch-order pre-pass (one classify kernel, 13 us on cfg2) on an auxiliary
                              stream, into one of three dispatch lists used in turn, so that it overlaps the PREVIOUS launches' tile
                              kernels on the caller's stream (the tile kernel waits for its list through an event): 0 = on the
                              caller's stream, in order (no second queue, no event; +4..5 us per cfg2 launch back to back), [1],
                              2 = as 1 with the auxiliary stream at the highest priority the device offers */
    MBK_OPT_EXACT_LONG,    /* group / scan pass 2: cap on exact_steps for the blocks that run 16-step groups (classified as
                              interior, where hardly any lane escapes early -- and one that does costs a trip plus the
                              block's single fix-up): [0] = no per-step prologue for them .. 4096 (cfg2 +0.4 %, inset +0.5 %) */
    MBK_OPT_SCAN_INLINE,   /* scan: when the host's probe of the window finds no pixel that outlives the light pass (an
                              all-exterior tile: 3 in 4 of a pyramid level), pass 1 finishes whatever blocks it cannot
                              finish in 4 steps itself, on the spot, stays in its block column, and pass 2 is not launched
                              (it cost 4.4 us to find empty lists): 0, [1] */
    MBK_OPT_WAVE_LIMIT,    /* asm/group and scan pass 2: cap on the resident waves per SIMD of the one-wave-per-block kernels,
                              imposed through unused dynamic LDS: [0] = none (8), 1..7.  Round 4 measured that the SIMD
                              arbiter serves its OLDEST wave first and that 2-3 waves saturate the fp64 pipe
                              (profiles/r04/valu_issue.txt): fewer resident waves shorten the drain at the end of a
                              launch but leave fewer slots to hide the latency of light blocks */
    MBK_OPT_UNITS_MIN_LIGHT, /* order 3: the units kernel serves a launch only when at least this share (x 65536) of the host's
                              probe pixels of the window is gone after 4 steps -- where there is little light area to batch, the
                              plain one-block-per-workgroup kernel (order 2) is the leaner one (cfg3: -0.7 %): 0 (always) ..
                              65536 [32768 = one half] */
    MBK_OPT_XCD_BALANCE,   /* order 3: shares of the eight XCDs in the units kernel's list of heavy blocks.  The XCDs of one chip run
                              2-10 % apart and the hardware deals them equal numbers of workgroups, so a launch lasts as long as
                              its slowest XCD: [0] even shares (default since round 5), 1 shares that follow the time stamps
                              earlier launches on the same stream left in pinned memory (72 stores per launch; the first launch
                              on a stream is even; only launches without the cycle test, and only those that had the chip to
                              themselves, are followed: strict cfg2 +0.7..1.2 %, nothing for the library's default path with
                              the cycle test or several tiles in flight -- which is why it is opt-in: bench.py times it beside its
                              headline, as `xcd_balance_opt_in`), 2 a fixed uneven deal (tests).  Changes when a block is computed,
                              never what is stored */
    MBK_OPT_M_LATE,        /* order 3: boundary blocks (centre pixel gone within the probe's 32 steps) whose centre escapes at
                              step >= this value open the dispatch order, before the interior blocks: the ~200 of them that
                              hold a never-escaping pixel run as long as an interior block and used to start a few microseconds
                              before the dispatchers ran dry (csrc/mbk_units.h): 0 (off: H, M, V), 1..65536 [8] -- a value above
                              MBK_OPT_PROBE_STEPS leaves the class empty (the probe reports no later step); the heavy-first
                              list of the launches the units kernel does not serve uses it when it lies in 2..probe_steps.
                              Changes when a block is computed, never what is stored */
    MBK_OPT_H_SETTLED,     /* order 3, with the cycle test only: interior blocks whose probe orbit is within 10^-k of settled (min over p of
                              |z_32 - z_(32-p)|^2 of the centre pixel) retire within a few checks, the others run (nearly) all
                              steps; the settled ones are dispatched behind the others, so that the last interior blocks to
                              start are short ones: 0 (one list), k = 1..30 [6].  Measured only together with M late
                              (profiles/r05).  Changes when a block is computed, never what is stored */
    MBK_OPT_CLASSIFY_WG,   /* order 3: threads per workgroup of the probe pre-pass, a multiple of 64: 64 .. [1024].  The pre-pass of launch
                              L + 1 runs beside the tile kernel of launch L (MBK_OPT_PREPASS_OVERLAP); a 1024-thread workgroup needs
                              16 free wave slots on ONE CU at once, which a chip full of single-wave workgroups offers only in its
                              drain */
    MBK_OPT_SCAN_STRIP,    /* scan, finish-in-place form (MBK_OPT_SCAN_INLINE; windows at least 512 pixels wide): a wave's region is 64 x 1
                              pixels instead of an 8x8 block, so that every store instruction writes one contiguous 256-byte
                              (int32) / 64-byte (uint8) piece of a row -- the all-exterior tile is bound by its stores, and a
                              store-only fill of the same box writes rows 1.5x (int32) / 2.5x (uint8) faster than 8x8 blocks
                              (profiles/r05/fill.txt): 0, [1].  Same loop, same arithmetic: which lane holds which pixel */
    MBK_OPT_CYCLE_WINDOW,  /* cycle test (MBK_OPT_CYCLE_DETECT): how the window of the saved reference state grows.  A pixel whose
                              orbit becomes bitwise periodic at step s retires at the first reference state taken after s (plus
                              lcm(8, period) steps); doubled windows (0: rounds 2-4) take them at steps 8, 16, 32, 64, ... -- 1.44 s
                              on average.  [32]: the window grows by a quarter (+ 1) while it is shorter than this many 8-step
                              checks and doubles from there on (long periods -- deep zooms -- need long windows): 6-7 % fewer
                              wave-steps on full-set views and shallow DataChunks, cfg3 unchanged (scripts/cycle_window_model.c).
                              0 .. 65536.  Every schedule is exact: a bitwise repeat proves the cycle whichever two steps match */
    MBK_OPT_SPILL_FIRST,   /* group, launches the units kernel does not serve (deep zooms; fp64 with 16-step groups, fp32; counts / bytes;
                              single-wave workgroups; dispatch order 2 or 3): SPILL (round 6, csrc/mbk_kernels.h block_pixel_spill,
                              csrc/mbk_spill.h).  A wave runs until its last lane is done, and on a deep zoom a third of the blocks
                              reach step ~500 with a handful of their 64 lanes alive.  At checkpoints -- this many steps after the
                              per-step prologue, then twice as far each time -- a block with at most MBK_OPT_SPILL_LANES live lanes writes
                              their state to a list in HBM and ends; a prefix sum compacts the list (no atomics) and a second kernel
                              runs the listed lanes 64 to a wave from where they stopped.  Same recurrence from the same state:
                              identical counts.  0 = off, else a multiple of 32 up to 65536 [256] */
    MBK_OPT_SPILL_LANES,   /* SPILL: a block spills when this many lanes or fewer are alive at a checkpoint (= the slots of 24 bytes a
                              block owns: state, lane / step word, list entry -- 403 MB for an 8192^2 window at 16): 1 .. 32 [16] */
    MBK_OPT_SPILL_MIN_MRD, /* SPILL: only launches with mrd at least this deep (shallow tiles have nothing to hand over): [2048] */
    MBK_OPT_SPILL_MIN_BLOCKS, /* SPILL: ... and only launches of at least 2^this 8x8 blocks: [19] = 5 800^2 pixels.  The second pass cannot
                              be shorter than one wave running the steps a never-escaping pixel has left (~ mrd x 21 ns: 0.2 ms at
                              mrd 10 000, 1 ms at 50 000) plus four small kernels (~30 us), while the first pass' saving grows with
                              the launch: below ~2^19 blocks the pass costs what it saves.  0 .. 31 */
    MBK_OPT_SPILL_CYC_SHIFT, /* SPILL with the cycle test: the second pass resumes orbits that have n steps behind them; the window of its
                              first reference state is n >> this checks (of 8 steps) instead of 1 -- [5]: where the schedule of an
                              unbroken run would stand (windows of ~ n / 4 steps); 31 = start at 1.  Any schedule is exact.  0 .. 31 */
    MBK_OPT_SURE_INTERIOR, /* group, strict fp64 launches (no cycle test, 16-step groups, mrd >= 65; csrc/mbk_kernels.h block_pixel,
                              csrc/mbk_loops.inc escape_steps_sure).  A block of the interior class whose 64 pixels all lie inside the
                              main cardioid or the period-2 disk by a margin of 1e-4 (two closed forms, mbk_sure_interior_point below)
                              runs its mrd - 1 steps with NO bailout test -- 6 issue slots per step instead of 6.125 -- and is tested
                              once behind the last step; "|z|^2 >= 4 stays >= 4" makes that one NaN-inclusive test stand for all the
                              others.  A wave whose test trips computes its block again the usual way, so the certificate only
                              predicts and never decides a result: identical counts, bytes and smooth values.  A launch whose window
                              holds no certified pixel (deep zooms, exterior tiles: a host probe) does not evaluate it.
                              [0] off, 1 on, 2 force: every block of the interior class takes the test-free loop whatever the
                              certificate says (for tests of the fallback; slower) */
    MBK_OPT_COUNT_
};
/* Read-only diagnostics through mbk_get_option: what hipOccupancyMaxActiveBlocksPerMultiprocessor reports for the
 * four scan-path kernels, in single-wave workgroups per CU: +0 f64 scan, +1 f64 heavy, +2 f32 scan, +3 f32 heavy. */
#define MBK_INFO_SCAN_WG_PER_CU 100
/* MBK_OPT_XCD_BALANCE = 1, of the stream that has reported most: +0..+7 the share of XCD x of the heavy list (x 2^20; an even
 * deal is 131072), +8 the number of the last launch whose time stamps were read, +9 the units launches issued. */
#define MBK_INFO_XCD_SHARE 110
/* SPILL (MBK_OPT_SPILL_FIRST): +0 the lanes the last launch with a second pass handed over to it (waits for that launch),
 * +1 the number of launches of this ctx that ran with one. */
#define MBK_INFO_SPILL 130
int mbk_set_option(mbk_ctx *ctx, int option, uint32_t value);
int mbk_get_option(mbk_ctx *ctx, int option, uint32_t *value);

/* Diagnostics of the units kernel's deal across the eight XCDs (MBK_OPT_XCD_BALANCE), on the host, without a device or a
 * context: the functions the kernels call.  mbk_units_plan: the shares for a list of n_h heavy entries, n_m middle entries
 * and n_v row units under the H fractions `fractions[8]` (sum 1) -> plan[40] ([2] = number of workgroup ids, [8 + x] /
 * [16 + x] = heavy / light entries of XCD x).  mbk_units_lookup: what workgroup id `id` computes: *list = 0 nothing, 1 heavy
 * entry *index, 2 middle entry *index, 3 row unit *index.  Every entry of every list is taken by exactly one id. */
int mbk_units_plan(uint32_t n_h, uint32_t n_v, uint32_t n_m, const double *fractions, uint32_t *plan);
int mbk_units_lookup(const uint32_t *plan, uint32_t id, uint32_t *list, uint32_t *index);

/* MBK_OPT_SURE_INTERIOR on the host, without a device or a context: the function the kernels call and what the host makes of it.
 * mbk_sure_interior_point: 1 when c = (cr, ci) passes the certificate -- q (q + x) < ci^2 / 4 - 1e-4 with x = cr - 1/4,
 * q = x^2 + ci^2 (main cardioid), or (cr + 1)^2 + ci^2 < 1/16 - 1e-4 (period-2 disk); binary64, every operation rounded on
 * its own -- else 0.  mbk_sure_interior_blocks: how many 8x8 blocks of the view's window a launch would certify (blocks wholly
 * inside the window that hold no pinned last sample of an axis, all 64 pixels passing).  mbk_sure_interior_flag: the word a
 * launch of that window carries to its kernel under MBK_OPT_SURE_INTERIOR = option and MBK_OPT_CYCLE_DETECT = cycle_detect
 * (flags: MBK_PRECISION_F32 or 0): 0 = no block evaluates the certificate, else the option's value. */
int mbk_sure_interior_point(double cr, double ci);
int mbk_sure_interior_blocks(const mbk_view *view, uint64_t *certified);
int mbk_sure_interior_flag(const mbk_view *view, uint32_t mrd, uint32_t flags, uint32_t cycle_detect, uint32_t option,
                           uint32_t *flag);

/* The quantiser alone, on the device: h_bytes[i] = uint8(ceil(h_counts[i] * 256 / mrd)) for n host counts
 * (WorkerCUDA.py:96-98; each count must lie in [0, mrd-1], which is what calc_mb_value returns).
 * Exists so that the exactness of the device's division-free form can be checked for every count. */
int mbk_quantise_counts(mbk_ctx *ctx, const int32_t *h_counts, uint64_t n, uint32_t mrd, uint8_t *h_bytes);

/* Device-side reduction over int32 counts already in HBM (asynchronous part on hip_stream -- NULL =
 * the null stream -- then a stream sync): fills stats->pixel_iterations and stats->never_pixels.  Used by bench.py to turn
 * kernel time into pixel-iterations/s from the kernel's own output. */
int mbk_reduce_counts(mbk_ctx *ctx, const int32_t *d_counts, uint64_t n, uint32_t mrd,
                      void *hip_stream, mbk_stats *stats);

/*
 * The worker loop in native code: lease -> compute -> send, pipelined, until the Distributer answers 0x11
 * ("no workload available") or max_tiles (0 = no limit) have been leased.  Replaces the loop of the reference worker,
 * WorkerCUDA.py:111-184 (do_workload_single called from main until it returns False), speaking the protocol of
 * Distributer.cs:30-45,358-458 / DistributerWorkload.cs:53-100 UNCHANGED: per tile the wire sees exactly the
 * reference's two exchanges (request 0x00 -> 0x10 + 4 x u32 | 0x11; response 0x01 + 4 x u32 -> 0x20 | 0x21, then on
 * 0x20 exactly MBK_CHUNK_BYTES raw bytes); only their timing overlaps with other tiles': while tile n is on the GPU
 * (slot n % MBK_SLOTS, its D2H overlapping the other slots' kernels) tile n+1 is being leased and tiles <= n-1 are being sent
 * by `senders` threads (1..64) on their own connections.  `senders + MBK_SLOTS` pinned 16 MiB buffers circulate, so a slow
 * server back-pressures the lease rate.  Uniform tiles (all 0 / all 1) are not copied off the GPU: their payload
 * comes from a shared constant buffer.  A rejected tile (0x21) is dropped and the loop carries on (WorkerCUDA.py:
 * 161-163).  On a socket error while leasing the loop stops leasing, finishes the tiles it holds, and returns
 * MBK_ERR_NET (mbk_last_error has the text).  The same single-host-thread rule as everything else on a ctx: the
 * calling thread drives the GPU; the sender threads touch sockets and host buffers only.
 * distributedmandelbrot_amd/worker.py: run_native / run_farm bind it; run_pipelined is the same loop in Python.
 */
typedef struct mbk_worker_report {
    uint64_t leased;           /* tiles obtained with opcode 0x00 */
    uint64_t accepted;         /* 0x20 and every payload byte handed to the socket */
    uint64_t rejected;         /* 0x21 */
    uint64_t resets;           /* 0x20, then the server reset the connection mid-payload (the reference server reads the
                                  payload with ONE Receive and closes, Distributer.cs:416-423: the tile is complete there) */
    uint64_t uniform_tiles;    /* sent from the shared constant buffer */
    uint64_t pixel_iterations; /* reference-equivalent, summed over the tiles */
    double kernel_ms_sum;
    double seconds;            /* wall time of the call */
    uint64_t net_retries;      /* exchanges that were repeated after a transient network failure (round 4, ABI 4) */
} mbk_worker_report;
int mbk_worker_run(mbk_ctx *ctx, const char *addr, uint16_t port, uint64_t max_tiles, uint32_t senders,
                   mbk_worker_report *report);

/*
 * Process-wide network behaviour of mbk_worker_run / mbk_feeder_run (every feeder of a farm shares it; round 4).  Why:
 * the reference Distributer accepts on ONE thread, one connection at a time, with a listen backlog of 16
 * (Distributer.cs:16,221,226-297) and 100 ms receive timeouts (:17,196-202), and the reference worker opened one
 * connection at a time (WorkerCUDA.py:115,148).  8 feeders x (4 senders + 1 lease connection) must not present that
 * server with 40 concurrent connects -- a full backlog is an RST on a Windows/.NET host -- and a computed tile must
 * not be dropped because one connect failed.  Both exchanges are retried with exponential backoff on transient
 * failures (refused, reset, timed out, closed before the reply) until the server has answered; after 0x20 the payload
 * is sent once (the server removed the lease when it accepted, Distributer.cs:404-423).
 */
enum mbk_net_option {
    MBK_NET_MAX_CONNECTIONS = 0,    /* connections open or being opened at any time, whole process; 1..64, default 8 */
    MBK_NET_CONNECT_TIMEOUT_MS = 1, /* 0 = wait for ever; default 10 000 */
    MBK_NET_IO_TIMEOUT_MS = 2,      /* per send / receive call without progress; 0 = none; default 30 000 */
    MBK_NET_RETRIES = 3,            /* attempts after the first, per exchange; 0..100, default 6 */
    MBK_NET_BACKOFF_MS = 4,         /* first pause; doubles per attempt up to 2 s, plus jitter; 1..10 000, default 50 */
    MBK_NET_STOP = 5,               /* 1: every running loop stops leasing, returns the tiles it holds and ends (Ctrl-C
                                       handlers set it from another thread); 0 re-arms */
    MBK_NET_PEAK_CONNECTIONS = 6,   /* read-only (mbk_net_get_option): the most connections that were ever open at once;
                                       setting MBK_NET_MAX_CONNECTIONS clears it */
    MBK_NET_FEEDER_SLOTS = 7,       /* tiles mbk_feeder_run keeps on its backend at once (slot numbers 0 .. k-1); 1..8, default 2 */
    MBK_NET_OPT_COUNT_
};
int mbk_net_set_option(int option, uint32_t value);
int mbk_net_get_option(int option, uint32_t *value);

/* The same protocol loop over a caller-supplied compute backend (mbk_worker_run is this with the backend bound to a
 * GPU context: submit = mbk_datachunk_submit_ex(MBK_LAZY_UNIFORM), wait = mbk_wait, alloc/release = pinned memory).
 * For hosts that schedule the GPU themselves, and for the CPU tests of the protocol engine.  submit / wait are
 * called from the calling thread only, with slot cycling through 0 .. k-1 (k = MBK_NET_FEEDER_SLOTS, default 2; mbk_worker_run uses MBK_SLOTS); wait must fill stats (all_bytes_zero /
 * all_bytes_one decide whether h_bytes or a constant buffer is sent).  on_tile (optional) is called from a sender
 * thread once per returned tile with status 1 accepted, 0 rejected, 2 reset after 0x20, -1 error. */
typedef struct mbk_feeder_ops {
    void *user;
    int (*submit)(void *user, int slot, uint32_t level, uint32_t mrd, uint32_t index_real, uint32_t index_imag, uint8_t *h_bytes);
    int (*wait)(void *user, int slot, mbk_stats *stats);
    void *(*alloc)(void *user, uint64_t bytes);
    void (*release)(void *user, void *ptr);
    void (*on_tile)(void *user, const uint32_t workload[4], const mbk_stats *stats, int status);
} mbk_feeder_ops;
int mbk_feeder_run(const mbk_feeder_ops *ops, const char *addr, uint16_t port, uint64_t max_tiles, uint32_t senders,
                   mbk_worker_report *report);

#ifdef __cplusplus
}
#endif
#endif /* MBK_H */
