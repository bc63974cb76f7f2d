#!/usr/bin/env python3
"""bench.py -- headline benchmark of the Mandelbrot tile escape-time path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg2] [--kernel default] [--shard own|queue|bands]
                    [--full] [--dump-outputs DIR]

A plain run does only what the headline needs: set up, ramp the clock, W warm-up steps, the K timed steps, one reduction
of the last step's counts (the pixel-iterations `value` counts), the line.  Everything else described below -- the
per-launch event pass, `output_verified`, the cycle-test leg, the SMI readings, the extra objects of N = 1 and
`cpu_baseline` -- runs only with `--full`.  `--dump-outputs DIR` (--shard own) writes what the last timed step computed:
counts.npy (float32; the int32 escape indices), nu.npy (float64; cfg5) and bytes.npy (float32; --outputs both), every
pixel in row-major order or, beyond 48 MiB in all, the same seeded sample of pixels in each (`outputs_dumped` in the line).

One "step" = one pass of the hot path over one batch of synthetic input already described in HBM terms: the
kernel generates its coordinates itself and writes int32 escape indices to a resident HBM buffer
(nothing crosses PCIe inside the timed region).  Workload: BASELINE.json configs[1] ("cfg2"): 4096x4096
samples of the full set (centre -0.5+0i, span 3.0), max_iter (mrd) = 1000, fp64.

N = 1 (the contract's headline): one cfg2 tile per step, launches back to back on one stream, one pair of HIP
events around the timed region (`--shard own`).

N > 1: `python bench.py --gpus N` starts its own N ranks (one process per GPU; RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* in the environment, exactly what `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`
sets -- that launcher works too and is detected by WORLD_SIZE).  Tiles are independent, so there is no data-path
collective and no RCCL anywhere: the only communication is a barrier, the max-over-ranks of the elapsed time and
a few gathered Python objects, on gloo (`--control nccl` exists to A/B that choice).  Three ways to shard:

  --shard queue (default for N > 1; strong scaling -- the north star's partition: "DataChunk tiles sharded across
                the GPUs by a plain per-GPU work queue", the shape of Distributer.cs:335-392 where many clients pull
                from one hand-out loop).  The job of one step is a FIXED set of T = grid x grid DataChunk-sized
                (4096x4096) tiles covering the workload's view at grid-times finer pitch (default 8 x 8 = 64 tiles:
                far exterior, boundary and all-interior tiles mixed, cost ratio > 100x).  Every rank pulls ticket
                numbers from ONE cursor in shared memory (sharding.SharedCursor), ticket t = tile t mod T of step
                t div T, four tiles in flight per GPU, tickets running on across steps (no barrier between steps).
                Rank 0 checks that every ticket was taken exactly once (`tiles_exactly_once`) and reports
                `tiles_per_rank`, the ranks' finish times and `ranks_seen` (host, pid, GPU name, PCI bus id of
                every rank: there is no RCCL to ask whether N distinct GPUs took part).
  --shard own   (default for N = 1; weak scaling): every rank computes its own cfg2 tile per step.
  --shard bands (strong scaling of ONE view, BASELINE cfg3's form): one view per step, cut into >= 16 row bands per
                GPU (of >= 128 rows) pulled from the same kind of cursor, two bands in flight per GPU.

Before the W warm-up steps the clock is pre-conditioned for --ramp-ms (150 ms) with untimed launches of
the same workload: an idle MI355X needs 50-100 ms of load to reach its sustained clock, and a 0.6 ms tile
measured cold reads 15-20 % low.  Round 6: EVERY leg of the line gets that ramp (each one
follows host work -- a reduction, a sha256 of 64 MiB, a sub-process -- through which the GPU idled: 20 ms of idleness
cost the next 60 launches 8 % on average, profiles/r06/burst_probe_0.txt; round 5's cycle-test, two-stream and
per-launch figures in the driver's 20-step run were measured that way and read 12-22 % low), and every leg beside
the headline is repeated until it holds >= 50 ms of device time (`steps_run`; the headline times exactly --steps).

Prints ONE JSON line on rank 0.  `value` = whole-job G pixel-iterations/s where a pixel's iterations
are count if count > 0 else mrd-1, summed from the kernel's own output.
`roofline`: the path is bound by the fp64 vector-ALU issue rate (not HBM, not MFMA -- FMA contraction
is forbidden by bit-exactness): achieved = 8 algorithmic flops per pixel-iteration / average
launch duration (HIP events on the launch stream); peak = CUs x 4 SIMD x 16 fp64 lanes x 2 flop x
clock (78.6 TFLOP/s on MI355X).  Under parity the default kernel needs 6.125 fp64-rate VALU issue
slots per 8 flops (6 arithmetic ops per step + one add and one compare per 16 steps), so the flops
fraction cannot exceed 8/12.25 = 0.653; `valu_slot_util` (= issue slots actually spent per
pixel-iteration over the 39.3 T lane-op/s issue peak at 2.4 GHz) is the "how close to the metal"
figure.  `traffic` is HBM bytes per launch from separate `rocprofv3 --pmc` passes of this same command
(committed under profiles/, see `traffic_source`); counters cannot be read from inside the run, so the
committed summary carries a hash of the kernel sources it was collected on and `traffic` is null when the
sources in the tree differ from it (a stale profile must not be quoted for a changed kernel).
`cpu_baseline`: the strict-IEEE C oracle (oracle/, kind "port": the reference has no CPU
implementation and its numba path cannot run here) on the host cores, rank 0, N = 1 only.

Cycle test: the library's default (MBK_OPT_CYCLE_DETECT = 1) retires a pixel as "never escapes" as soon as
its (zr, zi) bit pattern repeats -- bit-identical counts, but iterations the reference would run are not
executed.  `value` and `roofline` are therefore measured with the test OFF (every iteration executed; stated
in config.cycle_test); the same K steps with the default ON are timed right after in the same run and
reported as the extra object `cycle_detection` (reference-equivalent rate, ms per step, speed-up).
`--opt cycle_detect=1` moves the test into the headline, labelled as such.

`output_verified` (round 5): sha256 of the int32 counts the LAST TIMED launch wrote (one D2H after the timed region) and
the two totals against the CPU oracle's, committed in tests/golden/bench_outputs.json -- the number on the line belongs to
the reference's output inside this very run; the cycle-test leg carries its own.  `configs` (round 5, the default N = 1
line only): a short strict leg of every other single-GPU BASELINE config -- cfg3 (2 launches), cfg5 (3), DataChunk (1,0,0)
(20), cfg4 as one 16 384 x 1 024 band in fp32 (2) -- each with value, ms_per_step, roofline.frac and output_verified.

Round 6 also: the headline runs the library's DEFAULT options (the cycle test is the only one the leg changes;
MBK_OPT_XCD_BALANCE, which rounds 4-5 switched on for it, is timed as the extra object `xcd_balance_opt_in`);
`cycle_detection` carries `kernel_ms_avg` from one pair of HIP events around its launches beside the wall-clock
`ms_per_step`, and the host's submit time per launch; `sustained` = the headline's launches back to back for >= 1 s
with board power and shader clock sampled through librocm_smi64 (start / middle / end); `config.versions` = ROCm, HIP
runtime, kernel, VBIOS and firmware of the box.

More extra objects at N = 1, all outside `value` (SURVEY.md 8d "reported beside it"):
`end_to_end` -- a whole level of the reference's pyramid (level 16, mrd 1024: 256 DataChunk tiles) through the
host-buffer API, i.e. kernel + quantise + statistics + D2H into pinned memory: tiles/s synchronous, with two / three (the
worker loops' depth) / four tiles in flight, and with uniform tiles not copied (what the worker does); kernel median / mean / max, D2H mean;
`queue_job` -- the N > 1 default job (--shard queue) run on this one GPU, i.e. the same-mode N = 1 point of the
scaling curve.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

WORKLOADS = {
    # name: (start_r, start_i, range, width, height, mrd, description)
    "cfg1": (-2.0, -1.5, 3.0, 512, 512, 256, "512x512 full set (centre -0.5+0i, span 3.0), mrd 256"),
    "cfg2": (-2.0, -1.5, 3.0, 4096, 4096, 1000, "4096x4096 full set (centre -0.5+0i, span 3.0), mrd 1000"),
    "cfg3": (-0.743648, 0.131820, 1e-5, 8192, 8192, 10000,
             "8192x8192 deep zoom (centre -0.743643+0.131825i, span 1e-5), mrd 10000"),
    "chunk_l1": (-2.0, -2.0, 4.0, 4096, 4096, 1000, "DataChunk (level 1, 0, 0) = [-2,2]^2, mrd 1000"),
    # diagnostics (not BASELINE configs): uniform all-in-set tile = pure loop throughput, no divergence
    "inset": (-0.2, -0.1, 0.2, 4096, 4096, 1000, "4096x4096 inside the main cardioid (every pixel runs mrd-1 steps)"),
    "exterior": (-2.0, -2.0, 1.0, 4096, 4096, 1000, "DataChunk (4,0,0): every pixel escapes within 3 steps"),
    # BASELINE configs[3]: centre/span are not given there; SURVEY 8(d) proposes centre -0.745+0.11i, span 0.02
    "cfg4": (-0.755, 0.10, 0.02, 16384, 16384, 50000,
             "16384x16384 seahorse valley (centre -0.745+0.11i, span 0.02), mrd 50000, fp32 kernel variant"),
    # BASELINE configs[4]: no view given; the full-set view of cfg2 with the continuous value as output
    "cfg5": (-2.0, -1.5, 3.0, 4096, 4096, 5000,
             "4096x4096 full set (centre -0.5+0i, span 3.0), mrd 5000, continuous (smooth) colouring: float64 nu + int32 count per pixel"),
}
DEFAULT_PRECISION = {"cfg4": "f32"}
SMOOTH_WORKLOADS = {"cfg5"}
FLOPS_PER_PIXEL_ITER = 8        # 4 mul + 4 add/sub with the squares shared
# fp64-rate VALU issue slots each kernel spends per pixel-iteration (v_cmp costs a full slot on gfx950):
#   per-step test: 3 mul + 3 add + 1 fma + 1 v_cmp = 8;  grouped test: 6 + 2 per group = 6.25 (8-step groups,
#   kernel "refill" and option group_steps=8) or 6.125 (16-step groups: the default for interior blocks)
VALU_SLOTS_PER_PIXEL_ITER = {"default": 6.125, "scan": 6.125, "group": 6.125, "refill": 6.25, "asm": 8.0, "simple": 8.0}
# default (steps, warmup) per workload: enough launches for a steady clock, a few seconds at most
DEFAULT_STEPS = {"cfg1": (400, 50), "cfg2": (400, 50), "chunk_l1": (400, 50), "inset": (60, 8), "exterior": (400, 50),
                 "cfg3": (20, 3), "cfg4": (3, 1), "cfg5": (40, 5)}
# CPU baseline sample: every `stride`-th 8-row band, sized for ~10-30 CPU-seconds on >= 64 host threads
CPU_SAMPLE_STRIDE = {"cfg4": 256}
# Short strict legs of the other single-GPU BASELINE configs inside the default `python bench.py` line (object `configs`;
# VERDICT r4 item 2): name -> (workload, window (col0, row0, ncols, nrows) | None, timed launches, warm-up launches)
EXTRA_CONFIGS = {"cfg3": ("cfg3", None, 2, 1), "cfg5": ("cfg5", None, 3, 1), "chunk_l1": ("chunk_l1", None, 20, 5),
                 "cfg4_band": ("cfg4", (0, 7680, 16384, 1024), 2, 1)}
MIN_LEG_MS = 50.0   # every leg beside the headline is repeated until it holds at least this much device time (its `steps_run`)
SUSTAINED_S = 1.0   # the `sustained` object: the headline's launches back to back for at least this long, clock and power sampled
GOLDEN_OUTPUTS = os.path.join(ROOT, "tests", "golden", "bench_outputs.json")   # made by tests/golden/make_bench_golden.py
DUMP_BUDGET_BYTES = 48 * 2 ** 20   # --dump-outputs: at most this much in all; a seeded sample of the pixels beyond it
DUMP_SEED = 1000
PMC_SUMMARIES = [("r06", "cfg2_default_pmc_summary.json"), ("r05", "cfg2_default_pmc_summary.json"), ("r04", "cfg2_default_pmc_summary.json"), ("r03", "cfg2_default_pmc_summary.json"), ("r02", "cfg2_default_pmc_summary.json"), ("r01", "cfg2_default_pmc_summary.json")]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: per workload, ~0.3-6 s of GPU time)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default: per workload)")
    ap.add_argument("--ramp-ms", type=float, default=150.0,
                    help="untimed clock pre-conditioning before the warm-up steps: the same launches are repeated "
                         "for this long so that DVFS has left its idle state (an MI355X needs ~50-100 ms of load to "
                         "reach its sustained clock; a 0.6 ms tile measured cold reads 15-20 %% low). 0 disables.")
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS))
    ap.add_argument("--kernel", default="default")
    ap.add_argument("--precision", default=None, choices=["f64", "f32"],
                    help="f32 = BASELINE cfg4's fp32 kernel variant (not in the reference); default f64, cfg4: f32")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="library tuning option (include/mbk.h enum mbk_option), e.g. --opt group_steps=8; repeatable")
    ap.add_argument("--outputs", default="counts", choices=["counts", "both"],
                    help="counts (default, the contract's workload): int32 escape indices. both: also the quantised "
                         "uint8 tile the worker sends (what a DataChunk launch writes), for kernel studies")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline as well: output_verified against the CPU oracle's hashes, the "
                         "per-launch event pass (kernel_ms_median / min), the cycle-test leg, SMI readings and box versions, "
                         "at N = 1 the extra objects (sustained, xcd_balance_opt_in, two_streams, end_to_end, queue_job, "
                         "configs) and cpu_baseline.  Off: the line holds the headline and what the timed steps give")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step computed as DIR/<name>.npy (float32 / "
                         "float64; a fixed, seeded sample of the pixels when the whole would exceed 48 MiB); --shard own only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip cpu_baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full, N = 1: skip the end_to_end and queue_job objects (kernel studies, profiling passes)")
    ap.add_argument("--shard", default=None, choices=["own", "tiles", "queue", "bands"],
                    help="own (default for N = 1; 'tiles' is its old name): every rank computes its own tile per step "
                         "(weak scaling). queue (default for N > 1): one step = a fixed set of grid x grid 4096^2 tiles "
                         "that the ranks pull from a shared-memory cursor (strong scaling; the per-GPU work queue of the "
                         "north star). bands: ONE view per step, cut into >= 16 row bands per GPU pulled from the cursor "
                         "(strong scaling; how BASELINE cfg3 shards an image over 8 GPUs)")
    ap.add_argument("--queue-order", default="image", choices=["image", "longest"],
                    help="--shard queue: the order in which the tiles of a step are handed out.  image (default since round 5): the "
                         "order a Distributer walks its own list in (Distributer.cs:335-353) -- what a deployment gets.  longest: by "
                         "the census' pixel-iterations, longest first (rounds 3-4's default: the ranks finish together, which a real "
                         "server does not arrange; ADVICE r4)")
    ap.add_argument("--queue-order-image", action="store_true", help=argparse.SUPPRESS)   # (round 4's flag: now the default)
    ap.add_argument("--grid", type=int, default=8, help="--shard queue: the job is grid x grid tiles (default 8 -> 64 tiles per step)")
    ap.add_argument("--band-rows", type=int, default=0, help="rows per band for --shard bands (default: height / (16 N), >= 128)")
    ap.add_argument("--streams", type=int, default=None,
                    help="tiles (or bands) in flight per GPU (default 1 for own = the contract's serial steps, 2 for queue / bands)")
    ap.add_argument("--control", default="gloo", choices=["gloo", "nccl"],
                    help="backend of the barrier / timing reductions for N > 1 (no data-path collective exists)")
    ap.add_argument("--launch-events", default="region", choices=["region", "per-launch"],
                    help="--shard own: where the HIP events of the timed region sit.  region (default): ONE pair around the K "
                         "launches on the launch stream -- the average launch duration is its elapsed time / K, gaps between "
                         "launches included; median / minimum come from a separate untimed pass with a pair per launch.  "
                         "per-launch: a pair around every launch inside the timed region (rounds 1-3): each event is a "
                         "barrier packet in the queue, which costs the back-to-back launches ~2 %% (profiles/r04/NOTES.md)")
    ap.add_argument("--no-solo", action="store_true",
                    help="N > 1, queue / bands: skip the single-GPU pass of the same job that rank 0 runs alone after the "
                         "timed region (`single_gpu_same_job`; it takes N times as long as the timed region)")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="functional test only: rank r uses GPU r mod (visible GPUs), so that the N > 1 path can be "
                         "exercised on a box with fewer GPUs than ranks (labelled in config; never a scaling number)")
    args = ap.parse_args(argv)
    if args.shard == "tiles":
        args.shard = "own"
    if args.steps is not None and args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def self_launch(args) -> int:
    """`python bench.py --gpus N` outside any launcher: start the N ranks ourselves -- one process per GPU with the
    environment torch.distributed's env:// rendezvous reads (what torch.distributed.run would set), wait for all
    of them, and pass rank 0's stdout (the one JSON line) through.  If a rank dies the others are stopped (exact
    PIDs only) and the exit code is that rank's."""
    import socket
    import subprocess
    with socket.socket() as s_:            # a free rendezvous port
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MBK_BENCH_RUN_ID=f"{os.getpid()}")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))

    def forward():   # rank 0's JSON line goes to stdout; library chatter that lands on its stdout (gloo) to stderr
        for line in procs[0].stdout:
            (sys.stdout if line.startswith("{") else sys.stderr).write(line)
            sys.stdout.flush()

    import threading
    fwd = threading.Thread(target=forward, daemon=True)
    fwd.start()
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                print(f"bench.py: rank {procs.index(p)} exited with code {code}; stopping the other ranks", file=sys.stderr)
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    fwd.join(timeout=10)
    return rc


def cpu_baseline(name, workload, precision="f64"):
    """Time the C oracle (oracle/mandel_oracle.c, -ffp-contract=off) on the host cores."""
    from oracle.oracle import COracle
    sr, si, rng, w, h, mrd, _ = workload
    o = COracle()
    cores = o.max_threads()
    if name in SMOOTH_WORKLOADS:
        import numpy as np
        t0 = time.perf_counter()
        _, counts = o.view_smooth(sr, si, rng, rng, w, h, mrd)
        dt = time.perf_counter() - t0
        total = int(np.where(counts > 0, counts, mrd - 1).astype(np.int64).sum())
        return {"value": total / dt / 1e9, "unit": "G pixel-iterations/s", "cores": cores, "kind": "port",
                "sample": f"the whole {w}x{h} tile, mrd {mrd}, continuous value + count per pixel (mbo_view_smooth), "
                          "C oracle gcc -O2 -ffp-contract=off, OpenMP dynamic rows", "seconds": dt}
    # bounded sample: every `stride`-th row band of 8 rows, sized for roughly 10-30 CPU-seconds
    stride = CPU_SAMPLE_STRIDE.get(name, 1 if cores >= 4 else 4)
    bands = [(0, r, w, 8) for r in range(0, h, 8 * stride)]
    t0 = time.perf_counter()
    total = 0
    if stride == 1:
        _, _, total = o.view(sr, si, rng, rng, w, h, mrd, want_counts=False, want_bytes=False, nthreads=cores,
                             precision=precision)
        sample = f"the whole {w}x{h} tile, all rows"
        best_dt = time.perf_counter() - t0
        if best_dt < 2.0:   # short run: the first pass also pays for waking the OpenMP team; report the best of
            for _ in range(2):   # three passes (the baseline at its best, not at its worst)
                t1 = time.perf_counter()
                o.view(sr, si, rng, rng, w, h, mrd, want_counts=False, want_bytes=False, nthreads=cores, precision=precision)
                best_dt = min(best_dt, time.perf_counter() - t1)
            sample += " (best of 3 passes)"
    else:
        for win in bands:
            total += o.view(sr, si, rng, rng, w, h, mrd, window=win, want_counts=False,
                            want_bytes=False, nthreads=cores, precision=precision)[2]
        sample = f"every {stride}th 8-row band of the {w}x{h} tile ({len(bands) * 8} rows)"
        best_dt = time.perf_counter() - t0
    dt = best_dt
    rec = {"value": total / dt / 1e9, "unit": "G pixel-iterations/s", "cores": cores, "kind": "port",
           "sample": sample + f", mrd {mrd}, C oracle gcc -O2 -ffp-contract=off, OpenMP dynamic rows",
           "seconds": dt}
    if name in ("cfg3", "cfg4"):
        return rec       # one sample is already ~10 s of CPU
    # one thread, on every 16th 8-row band (the all-core figure above divided by `cores` hides the SMT/boost effects)
    t0 = time.perf_counter()
    tot1 = sum(o.view(sr, si, rng, rng, w, h, mrd, window=(0, r, w, 8), want_counts=False, want_bytes=False,
                      nthreads=1, precision=precision)[2] for r in range(0, h, 128))
    dt1 = time.perf_counter() - t0
    rec["single_thread"] = {"value": tot1 / dt1 / 1e9, "seconds": dt1, "sample": f"every 16th 8-row band ({h // 16} rows)"}
    if precision == "f64" and stride == 1 and o.have_avx512():
        # best-effort CPU: the same strict arithmetic 8 pixels at a time in AVX-512 (no fmadd), same threads
        dt8 = None
        for _ in range(3):   # best of three, as above
            t0 = time.perf_counter()
            _, total8 = o.view_avx512(sr, si, rng, rng, w, h, mrd, want_counts=False, nthreads=cores)
            dt8 = min(dt8, time.perf_counter() - t0) if dt8 is not None else time.perf_counter() - t0
        rec["best_effort_avx512"] = {"value": total8 / dt8 / 1e9, "seconds": dt8, "bit_identical_work": total8 == total}
    return rec



def kernel_source_hash():
    """sha256 over the HIP sources of libmbk_hip.so (what a committed PMC summary was collected on)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "distributedmandelbrot_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(csrc, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def pmc_traffic(workload, kernel):
    """(HBM bytes per launch, source) from the committed rocprofv3 PMC passes of this same command:
    WRITE_SIZE and FETCH_SIZE are in KiB, each collected in its own pass; FETCH_SIZE is doubled as
    MI355X_MICROARCH.md prescribes for gfx950.  (None, why) for un-profiled combinations and for a summary
    whose `source_sha256` is not the hash of the kernel sources in this tree (stale profile)."""
    if workload != "cfg2" or kernel not in ("default", "scan", "group"):
        return None, None
    have = kernel_source_hash()
    why = None
    for rnd, fname in PMC_SUMMARIES:
        path = os.path.join(ROOT, "profiles", rnd, fname)
        try:
            with open(path) as f:
                pmc = json.load(f)
            if pmc.get("source_sha256") != have:
                why = why or (f"profiles/{rnd}/{fname} was collected on other kernel sources (source_sha256 "
                              f"{str(pmc.get('source_sha256'))[:12]} != {have[:12]} in this tree): not quoted")
                continue
            nbytes = int(pmc["WRITE_SIZE"]["mean"] * 1024 + 2 * pmc["FETCH_SIZE"]["mean"] * 1024)
            return nbytes, f"profiles/{rnd}/{fname}: separate rocprofv3 --pmc passes of this command on these kernel sources, not counters of this run"
        except Exception:
            continue
    return None, why


def golden_outputs():
    try:
        with open(GOLDEN_OUTPUTS) as f:
            return json.load(f)
    except Exception:   # noqa: BLE001 -- a missing fixture is reported as "not verified", never fatal
        return {}


class SmiSampler:
    """Board power / shader clock of one GPU through librocm_smi64 (ctypes; the code of scripts/power_trace.py).  Every
    method returns None instead of raising: the line must not depend on the SMI library being usable on the box."""

    def __init__(self, index=0):
        import ctypes as C
        self.C, self.index, self.lib, self.cap_w = C, index, None, None

        class Freqs(C.Structure):
            _fields_ = [("has_deep_sleep", C.c_bool), ("num_supported", C.c_uint32), ("current", C.c_uint32),
                        ("frequency", C.c_uint64 * 33)]
        self.Freqs = Freqs
        try:
            lib = C.CDLL("librocm_smi64.so")
            if lib.rsmi_init(C.c_uint64(0)) == 0:
                self.lib = lib
                cap = C.c_uint64(0)
                if lib.rsmi_dev_power_cap_get(index, 0, C.byref(cap)) == 0:
                    self.cap_w = cap.value / 1e6
        except Exception:   # noqa: BLE001
            self.lib = None

    def sample(self):
        """(seconds, power W | None, sclk MHz | None)"""
        if self.lib is None:
            return None
        C = self.C
        try:
            p, typ = C.c_uint64(0), C.c_int(0)
            power = p.value / 1e6 if self.lib.rsmi_dev_power_get(self.index, C.byref(p), C.byref(typ)) == 0 else None
            f = self.Freqs()
            clk = (f.frequency[f.current] / 1e6 if self.lib.rsmi_dev_gpu_clk_freq_get(self.index, 0, C.byref(f)) == 0 and f.current < 33
                   else None)
            return time.perf_counter(), power, clk
        except Exception:   # noqa: BLE001
            return None

    def versions(self):
        out = {}
        if self.lib is None:
            return out
        C = self.C
        try:
            buf = C.create_string_buffer(128)
            if self.lib.rsmi_dev_vbios_version_get(self.index, buf, 128) == 0:
                out["vbios"] = buf.value.decode(errors="replace")
            for name, block in (("fw_mec", 5), ("fw_smc", 16), ("fw_rlc", 10), ("fw_sdma", 14)):   # rsmi_fw_block_t (rocm_smi.h)
                v = C.c_uint64(0)
                if self.lib.rsmi_dev_firmware_version_get(self.index, block, C.byref(v)) == 0:
                    out[name] = int(v.value)
        except Exception:   # noqa: BLE001
            pass
        return out

    def close(self):
        if self.lib is not None:
            try:
                self.lib.rsmi_shut_down()
            except Exception:   # noqa: BLE001
                pass
            self.lib = None

    def trace(self, period_s=0.02):
        """Start sampling in a thread; returns stop() -> list of samples."""
        import threading
        rows, stop = [], threading.Event()

        def poll():
            while not stop.is_set():
                r = self.sample()
                if r is not None:
                    rows.append(r)
                time.sleep(period_s)
        th = threading.Thread(target=poll, daemon=True)
        if self.lib is not None:
            th.start()

        def done():
            stop.set()
            if th.is_alive():
                th.join(timeout=1.0)
            return rows
        return done


def box_versions(torch, smi):
    """What the numbers of this line were measured on: ROCm release, HIP runtime, kernel / amdgpu driver, firmware."""
    out = {"hip_runtime": getattr(torch.version, "hip", None), "torch": torch.__version__, "kernel": os.uname().release}
    for key, path in (("rocm", "/opt/rocm/.info/version"), ("amdgpu_driver", "/sys/module/amdgpu/version")):
        try:
            with open(path) as f:
                out[key] = f.read().strip()
        except Exception:   # noqa: BLE001
            out[key] = None
    out.update(smi.versions())
    return out


def verify_output(name, d_counts, pixel_iterations, never_pixels, view, mrd, precision, window=None):
    """Pin a timed output inside this very run: sha256 of the int32 counts the launches wrote (one D2H) against the CPU
    oracle's (tests/golden/bench_outputs.json, made by tests/golden/make_bench_golden.py), plus the two totals."""
    import hashlib
    g = golden_outputs().get(name)
    if g is None:
        return {"verified": None, "why": f"no golden entry '{name}' in tests/golden/bench_outputs.json"}
    same_job = (list(g["view"]) == [view.start_r, view.start_i, view.range_r, view.range_i, view.width, view.height]
                and g["mrd"] == mrd and g["precision"] == precision
                and (tuple(g["window"]) if g["window"] else None) == (tuple(window) if window else None))
    if not same_job:
        return {"verified": None, "why": f"golden entry '{name}' describes another view / mrd / precision"}
    digest = hashlib.sha256(d_counts.cpu().numpy().data).hexdigest()
    ok = digest == g["counts_sha256"] and int(pixel_iterations) == g["pixel_iterations"] and int(never_pixels) == g["never_pixels"]
    return {"verified": bool(ok), "counts_sha256": digest, "sha256_matches": digest == g["counts_sha256"],
            "pixel_iterations_match": int(pixel_iterations) == g["pixel_iterations"],
            "never_pixels_match": int(never_pixels) == g["never_pixels"],
            "golden": f"tests/golden/bench_outputs.json['{name}'] (CPU oracle, {g['oracle']})"}


def dump_sample(npix, bytes_per_pixel, budget=DUMP_BUDGET_BYTES, seed=DUMP_SEED):
    """--dump-outputs: None (every pixel fits in `budget`) or the sorted pixel indices of a fixed, seeded sample of at most
    budget / bytes_per_pixel pixels -- the same indices for every output of a step and in every run with the same arguments:
    one pixel at a seeded random offset in every stride of ceil(npix / keep) pixels (increasing, hence unique)."""
    import numpy as np
    keep = budget // bytes_per_pixel
    if npix <= keep:
        return None
    stride = -(-npix // keep)
    base = np.arange(0, npix, stride, dtype=np.int64)
    return np.minimum(base + np.random.default_rng(seed).integers(0, stride, size=base.size, dtype=np.int64), npix - 1)


def dump_outputs(out_dir, outputs, npix):
    """Write what the last timed step computed, DIR/<name>.npy per output.  `outputs`: (name, flat device tensor of npix
    elements, numpy dtype float32 | float64).  A sample, when needed, is gathered on the device: one short D2H per output."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    idx = dump_sample(npix, sum(np.dtype(dt).itemsize for _, _, dt in outputs))
    d_idx = torch.from_numpy(idx).to(outputs[0][1].device) if idx is not None else None
    files = {}
    for name, t, dt in outputs:
        a = (t if d_idx is None else t[d_idx]).cpu().numpy().astype(dt)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        files[name] = {"dtype": np.dtype(dt).name, "elements": int(a.size)}
    return {"dir": out_dir, "files": files,
            "sample": None if idx is None else f"{idx.size} of {npix} pixels (bench.dump_sample: one at a seeded offset in every "
                                               f"stride of {-(-npix // idx.size)}), row-major pixel order"}


def extra_configs(dev, torch, gpu_index, device_info, ramp_ms=150.0):
    """Short strict legs (cycle test off, library defaults otherwise) of the other single-GPU BASELINE configs, so that the
    one command the driver times shows every one of them: per config `value`, `ms_per_step`, `roofline.frac` and
    `output_verified` (the timed launches' own buffer against the oracle's hash).  Not part of the headline `value`."""
    from distributedmandelbrot_amd import View
    out = {}
    stream = torch.cuda.current_stream()
    for name, (wl, window, steps, warm) in EXTRA_CONFIGS.items():
        try:
            sr, si, rng, width, height, mrd, desc = WORKLOADS[wl]
            precision = DEFAULT_PRECISION.get(wl, "f64")
            smooth = wl in SMOOTH_WORKLOADS
            view = View(sr, si, rng, rng, width, height)
            col0, row0, ncols, nrows = window if window else (0, 0, width, height)
            npx = ncols * nrows
            d_counts = torch.empty(npx, dtype=torch.int32, device=f"cuda:{gpu_index}")
            d_smooth = torch.empty(npx, dtype=torch.float64, device=f"cuda:{gpu_index}") if smooth else None

            def launch():
                if smooth:
                    dev.launch_view_smooth(view, mrd, d_smooth=d_smooth.data_ptr(), d_counts=d_counts.data_ptr(), stream=stream.cuda_stream)
                else:
                    dev.launch_view(view, mrd, window=window, d_counts=d_counts.data_ptr(), stream=stream.cuda_stream, precision=precision)

            sp0 = dev.spill_info() if hasattr(dev, "spill_info") else {"launches": 0}
            t_ramp = time.perf_counter()        # clock pre-conditioning, as for the headline (--ramp-ms): the legs before this
            while (time.perf_counter() - t_ramp) * 1e3 < ramp_ms:   # one left the GPU idle or on another kind of load
                launch()
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(warm):
                launch()
            e1.record(stream)
            torch.cuda.synchronize()
            # a timed region of at least MIN_LEG_MS of device time: `steps` is the floor, `steps_run` what ran
            steps_min, steps = steps, max(steps, int(-(-MIN_LEG_MS // max(e0.elapsed_time(e1) / max(warm, 1), 1e-3))))
            t0 = time.perf_counter()
            e0.record(stream)
            for _ in range(steps):
                launch()
            t_submit = time.perf_counter() - t0
            e1.record(stream)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ev_ms = e0.elapsed_time(e1) / steps
            st = dev.reduce_counts(d_counts.data_ptr(), npx, mrd, stream=stream.cuda_stream)
            cus, mhz = device_info["compute_units"], device_info["clock_mhz"]
            peak = cus * 4 * (16 if precision == "f64" else 32) * mhz * 1e6 * 2 / 1e12
            achieved = FLOPS_PER_PIXEL_ITER * st.pixel_iterations / (ev_ms / 1e3) / 1e12
            out[name] = {
                "workload": desc + (f"; rows {row0}..{row0 + nrows - 1} of it as one launch" if window else "")
                            + ("; int32 counts + float64 nu to resident HBM" if smooth else "; int32 counts to resident HBM"),
                "dtype": precision, "cycle_test": "off (every iteration executed)", "steps": steps_min, "steps_run": steps, "warmup": warm,
                "clock_ramp_ms": ramp_ms, "host_submit_us_per_launch": t_submit / steps * 1e6,
                "value": st.pixel_iterations * steps / wall / 1e9, "unit": "G pixel-iterations/s", "ms_per_step": wall / steps * 1e3,
                "pixel_iterations_per_step": st.pixel_iterations,
                "roofline": {"bound": "fp64_valu" if precision == "f64" else "fp32_valu", "achieved": achieved, "peak": peak,
                             "unit": "TFLOP/s", "frac": achieved / peak, "kernel_ms_avg": ev_ms,
                             "basis": "one pair of HIP events on the launch stream around the timed launches, elapsed / K"},
                "output_verified": verify_output(name, d_counts, st.pixel_iterations, st.never_pixels, view, mrd, precision, window),
            }
            try:   # SPILL (MBK_OPT_SPILL_FIRST): did the launches of this leg run with a second pass, and how many lanes did it take?
                sp1 = dev.spill_info()
                if sp1["launches"] > sp0["launches"]:
                    out[name]["second_pass"] = {"lanes_per_launch": sp1["lanes_last_launch"], "share_of_pixels": sp1["lanes_last_launch"] / npx,
                                                "what": "SPILL (include/mbk.h MBK_OPT_SPILL_FIRST, library default): blocks that reach a checkpoint "
                                                        "with <= 16 live lanes hand them to a second kernel that runs them 64 to a wave"}
            except Exception:   # noqa: BLE001
                pass
            del d_counts, d_smooth
        except Exception as e:   # noqa: BLE001 -- reported, must not cost the headline
            out[name] = {"error": repr(e)}
    return out


def end_to_end(dev, level=16, mrd=1024):
    """the tile rate INCLUDING quantise + statistics + D2H, reported beside the headline.  A whole
    level of the reference's pyramid (level n = n x n DataChunk tiles of [-2,2]^2, Distributer.cs:335-353 hands out
    every one of them) through the host-buffer API into pinned memory, library defaults (cycle test on):
    synchronous (WorkerCUDA.py:87-98's shape), two tiles in flight (rounds 1-4's pipeline) and MBK_SLOTS (4) in flight, each
    also with MBK_LAZY_UNIFORM (what worker.run_pipelined / mbk_worker_run do: uniform tiles are not copied off the GPU and
    tiles wholly outside |c| = 2 cost no GPU work)."""
    import numpy as np
    tiles = [(ir, ii) for ir in range(level) for ii in range(level)]
    n = len(tiles)
    pins = [dev.pinned_empty((16777216,), np.uint8) for _ in range(2)]
    dev.datachunk(level, mrd, 0, 0, out_bytes=pins[0])   # warm-up
    ks, ds, never, imm, iters = [], [], 0, 0, 0
    t0 = time.perf_counter()
    for ir, ii in tiles:
        _, _, st = dev.datachunk(level, mrd, ir, ii, out_bytes=pins[0])
        ks.append(st.kernel_ms)
        ds.append(st.d2h_ms)
        never += st.all_bytes_zero
        imm += st.all_bytes_one
        iters += st.pixel_iterations
    t_sync = time.perf_counter() - t0

    host_answered = [0]

    def in_flight(k, lazy):
        """the whole level with k tiles in flight: submit tile i on slot i % k, retire the oldest when all k are taken"""
        host_answered[0] = 0
        t1 = time.perf_counter()
        for i in range(n + k):
            if i >= k:
                st_ = dev.wait((i - k) % k)
                host_answered[0] += st_.kernel_ms == 0.0 and st_.d2h_ms == 0.0 and st_.all_bytes_one   # (no GPU work: ADVICE r5)
            if i < n:
                dev.submit_datachunk(i % k, level, mrd, *tiles[i], pins[i % k], lazy_uniform=lazy)
        return time.perf_counter() - t1

    nslots = int(getattr(dev, "SLOTS", 2))
    pins += [dev.pinned_empty((16777216,), np.uint8) for _ in range(nslots - len(pins))]
    def best(k, lazy):      # a pass takes 60-120 ms and the pool's boxes differ by +-5 % from one pass to the next: the better of two
        return min(in_flight(k, lazy), in_flight(k, lazy))
    t_two = best(2, False)
    t_lazy = best(2, True)
    t_three = best(min(3, nslots), False)      # what the worker loops keep in flight (round 6: the measured-best depth)
    t_three_lazy = best(min(3, nslots), True)
    t_all = best(nslots, False)
    t_all_lazy = best(nslots, True)
    ks_sorted = sorted(ks)
    return {"what": f"level {level} of the reference's pyramid, mrd {mrd}: {n} DataChunk tiles (4096^2) through the host-buffer "
                    "API on one context -- kernel + quantise + statistics + D2H of the 16 MiB byte tile into pinned memory, "
                    "library defaults (cycle test on); the pipelined rates are the better of two passes each; not part of `value`",
            "tiles": n, "uniform_never_tiles": int(never), "uniform_immediate_tiles": int(imm),
            "tiles_per_s_synchronous": n / t_sync, "tiles_per_s_two_in_flight": n / t_two,
            "tiles_per_s_two_in_flight_lazy_uniform": n / t_lazy,
            "tiles_per_s_three_in_flight": n / t_three, "tiles_per_s_three_in_flight_lazy_uniform": n / t_three_lazy,
            "worker_depth": min(3, nslots), "host_answered_tiles": int(host_answered[0]),
            "slots": nslots, "tiles_per_s_all_slots_in_flight": n / t_all, "tiles_per_s_all_slots_in_flight_lazy_uniform": n / t_all_lazy,
            "lazy_uniform": "MBK_LAZY_UNIFORM, what the worker loops use: a tile wholly outside |c| = 2 is answered on the host "
                            "(no GPU work: every count is 1 -- `host_answered_tiles` of them, counted in the lazy rates), a uniform "
                            "tile is not copied off the GPU",
            "G_pixel_iterations_per_s_wall_synchronous": iters / t_sync / 1e9,
            "kernel_ms_median": ks_sorted[n // 2], "kernel_ms_mean": sum(ks) / n, "kernel_ms_max": ks_sorted[-1],
            "d2h_ms_mean": sum(ds) / n}


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    fake_env = os.environ.get("MBK_BENCH_FAKE") == "1"
    if args.gpus > 1 and not args.oversubscribe and not fake_env:
        # one line instead of N ranks dying one by one: more ranks than GPUs is never a scaling number
        try:
            from distributedmandelbrot_amd import device_count
            visible = device_count()
        except Exception as e:   # noqa: BLE001
            raise SystemExit(f"bench.py: cannot count the GPUs ({e}); there is no CPU fallback")
        if args.gpus > visible:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but only {visible} GPU(s) visible on this node; one process per GPU is the "
                             "contract -- add --oversubscribe to exercise the N > 1 path on fewer GPUs (functional test, not a scaling number)")
    if args.gpus > 1 and world == 1:
        raise SystemExit(self_launch(args))     # start our own N ranks; each comes back here with WORLD_SIZE = N
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    fake = os.environ.get("MBK_BENCH_FAKE") == "1"   # CPU-only test hook for the N>1 control path
    if fake and os.environ.get("MBK_BENCH_FAKE_DIE_RANK") == str(rank):   # test hook: a rank that dies at start-up
        raise SystemExit(3)
    if args.shard is None:
        args.shard = "queue" if world > 1 else "own"
    own_mode, queue_mode, bands_mode = args.shard == "own", args.shard == "queue", args.shard == "bands"
    d_steps, d_warm = DEFAULT_STEPS.get(args.workload, (20, 3))
    if queue_mode:   # a step is grid^2 tiles, not one; the timed region keeps its length per GPU as N grows (the job of
        # a step is fixed -- strong scaling -- but more steps are timed: at N = 8 the 25 steps of N = 1 would last 0.1 s)
        d_steps, d_warm = max(2, d_steps * 4 // (args.grid * args.grid)) * world, 1
    if bands_mode:   # likewise: an image is a fixed job, the number of timed images grows with N
        d_steps *= world
    if args.steps is None:
        args.steps = d_steps
    if args.warmup is None:
        args.warmup = d_warm
    if args.precision is None:
        args.precision = DEFAULT_PRECISION.get(args.workload, "f64")
    smooth = args.workload in SMOOTH_WORKLOADS
    if args.streams is None:
        # in flight per GPU (r3, one MI355X): queue 1 / 2 / 3 / 4 -> 5 172 / 5 347 / 5 496 / 5 506 G/s; bands 3 is the knee
        args.streams = 1 if own_mode else 4 if queue_mode else 3
    if smooth and (not own_mode or args.precision != "f64"):
        raise SystemExit("cfg5 (smooth colouring) runs with --shard own in fp64")
    if args.grid < 1 or args.grid > 15:
        raise SystemExit("--grid must be in 1..15 (the grid view has grid x 4096 < 2^16 columns)")
    if args.dump_outputs and (not own_mode or fake_env):
        raise SystemExit("--dump-outputs needs --shard own on the GPU path (one tile per step: its buffers are the step's outputs)")
    options = {}
    for item in args.opt:
        k, _, v = item.partition("=")
        options[k] = int(v)

    import torch
    import torch.distributed as dist

    workload = WORKLOADS[args.workload]
    sr, si, rng, width, height, mrd, desc = workload
    npix = width * height

    backend = None
    gpu_index = local_rank
    if world > 1:
        if fake or args.control == "gloo":
            backend = "gloo"     # barrier + two scalar reductions on CPU tensors: nothing here needs RCCL
            dist.init_process_group(backend="gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
            backend = "nccl"
    if not fake and args.oversubscribe:
        gpu_index = local_rank % max(1, torch.cuda.device_count())

    def barrier():
        if world > 1:
            dist.barrier()

    def gather(obj):
        if world == 1:
            return [obj]
        out = [None] * world
        dist.all_gather_object(out, obj)
        return out

    nstreams = max(1, args.streams)
    # >= 16 bands per GPU, but no band under 128 rows: a band costs ~70 us of host work (cursor lock, two kernel
    # launches, an event), which must stay below its GPU time.  Tickets run on across steps (no barrier
    # between images), so the tail that larger bands leave idle is paid once per run, not once per image.
    band_rows = args.band_rows or max(128, height // (16 * world))
    band_rows = max(8, (band_rows // 8) * 8)
    from distributedmandelbrot_amd.sharding import Band, SharedCursor, make_bands
    bands = make_bands(height, band_rows) if bands_mode else None
    ntiles = args.grid * args.grid if queue_mode else 0
    units = bands if bands_mode else list(range(ntiles))     # what a ticket maps to (ticket mod len(units))
    cursor = None

    def open_cursor(tag):
        cname = (f"{tag}_{os.environ.get('MASTER_PORT', 'solo')}_"
                 f"{os.environ.get('MBK_BENCH_RUN_ID', os.environ.get('TORCHELASTIC_RUN_ID', os.getppid() if world > 1 else os.getpid()))}")
        c = SharedCursor(cname, create=True) if rank == 0 else None
        barrier()
        return c if rank == 0 else SharedCursor(cname, create=False)

    if bands_mode or queue_mode:
        cursor = open_cursor("b" if bands_mode else "q")

    dev = None
    me = {"rank": rank, "local_rank": local_rank, "host": os.uname().nodename, "pid": os.getpid()}
    if fake:
        device_info = {"name": "fake", "compute_units": 256, "clock_mhz": 2400}
        me.update(gpu_index=gpu_index, device="fake", pci_bus_id=None)
        streams = [None] * nstreams

        def launch_own(i):
            time.sleep(0.001)

        def launch_unit(i, u):   # stub cost: per band row / per tile class (so that a chunk of bands costs its rows)
            time.sleep(2e-6 * u.nrows if bands_mode else 0.0002 * (1 + u % 3))

        def unit_stats(u):          # (pixel-iterations, never-escaped pixels) of a queue tile
            return 10 ** 7 * (1 + u % 3), u % 3

        def sync():
            pass

        def slot_wait(i):
            pass
    else:
        from distributedmandelbrot_amd import MandelbrotDevice, View
        torch.cuda.set_device(gpu_index)
        dev = MandelbrotDevice(gpu_index)   # raises loudly without the HIP library / a gfx950 GPU
        # The headline is measured with the cycle test OFF: every iteration the reference would run is executed, so
        # `value` and the roofline describe the loop itself.  The library's default (ON: bit-identical counts, exactly
        # periodic orbits retired early) is timed in the same run as the extra object "cycle_detection".
        if "cycle_detect" not in options:
            dev.set_option("cycle_detect", 0)
        # Round 6: the headline runs the library's defaults -- the cycle test is the only option this leg
        # changes.  MBK_OPT_XCD_BALANCE (opt-in, library default 0; rounds 4-5 switched it on for this leg) is timed as an extra
        # object of its own, `xcd_balance_opt_in`, after the headline.
        for k, v in options.items():
            dev.set_option(k, v)
        device_info = dev.info()
        device_info["scan_occupancy"] = dev.scan_occupancy()
        me.update(gpu_index=gpu_index, device=device_info.get("name"), pci_bus_id=dev.pci_bus_id())
        view = View(sr, si, rng, rng, width, height)
        # --shard queue: grid x grid tiles of width x height samples = windows of ONE view of the same region at
        # grid-times finer pitch (np.linspace over the whole region, like every view of this library)
        qview = View(sr, si, rng, rng, width * args.grid, height * args.grid)
        nbuf = nstreams if (own_mode or queue_mode) else 1
        d_counts_all = [torch.empty(npix, dtype=torch.int32, device=f"cuda:{gpu_index}") for _ in range(nbuf)]
        d_smooth_all = [torch.empty(npix, dtype=torch.float64, device=f"cuda:{gpu_index}") for _ in range(nbuf)] if smooth else None
        d_bytes_all = [torch.empty(npix, dtype=torch.uint8, device=f"cuda:{gpu_index}") for _ in range(nbuf)] if args.outputs == "both" else None
        streams = [torch.cuda.current_stream()] + [torch.cuda.Stream() for _ in range(nstreams - 1)]
        slot_events = [torch.cuda.Event() for _ in range(nstreams)]
        slot_busy = [False] * nstreams

        def launch_own(i):
            if smooth:
                dev.launch_view_smooth(view, mrd, d_smooth=d_smooth_all[i].data_ptr(), d_counts=d_counts_all[i].data_ptr(),
                                       stream=streams[i].cuda_stream, kernel=args.kernel)
            else:
                dev.launch_view(view, mrd, d_counts=d_counts_all[i].data_ptr(), stream=streams[i].cuda_stream,
                                d_bytes=d_bytes_all[i].data_ptr() if d_bytes_all else 0,
                                kernel=args.kernel, precision=args.precision)

        def launch_unit(i, u):
            if bands_mode:   # a row band of the shared view, written at its place in this rank's image
                dev.launch_view(view, mrd, window=(0, u.row0, width, u.nrows),
                                d_counts=d_counts_all[0].data_ptr() + 4 * u.row0 * width,
                                stream=streams[i].cuda_stream, kernel=args.kernel, precision=args.precision)
            else:            # tile u of the grid, into this slot's own tile buffer
                tr, ti = u % args.grid, u // args.grid
                dev.launch_view(qview, mrd, window=(tr * width, ti * height, width, height),
                                d_counts=d_counts_all[i].data_ptr(), stream=streams[i].cuda_stream,
                                d_bytes=d_bytes_all[i].data_ptr() if d_bytes_all else 0,
                                kernel=args.kernel, precision=args.precision)
            slot_events[i].record(streams[i])
            slot_busy[i] = True

        def unit_stats(u):
            launch_unit(0, u)
            slot_wait(0)
            st = dev.reduce_counts(d_counts_all[0].data_ptr(), npix, mrd, stream=streams[0].cuda_stream)
            return st.pixel_iterations, st.never_pixels

        def slot_wait(i):          # back-pressure: one unit in flight per slot, or a rank would drain the cursor
            if slot_busy[i]:
                slot_events[i].synchronize()
                slot_busy[i] = False

        def sync():
            torch.cuda.synchronize()

        def ramp_clock():
            """Untimed clock pre-conditioning (--ramp-ms) with the launches of the leg that follows: every leg of this line
            comes after host work (a reduction, a hash of 64 MiB, a sub-process) during which the GPU idled and its clock fell;
            a 5 ms leg measured right after reads 10-20 % low (round 5's cycle-test and two-stream legs in the driver's run)."""
            t_r = time.perf_counter()
            while args.ramp_ms > 0 and (time.perf_counter() - t_r) * 1e3 < args.ramp_ms:
                launch_own(0)
                sync()

    turn = [0]
    my_tickets = []
    launches = [0]

    def run_steps(nsteps, events=None, pullers=world):
        """own: nsteps launches round-robin over the streams.  queue / bands: pull tickets until nsteps steps are done
        (`pullers` = the ranks pulling from the cursor: it sizes the guided chunks of the bands mode)."""
        if own_mode:
            region = events is not None and not fake and args.launch_events == "region" and nstreams == 1
            if region:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(streams[0])
            for _ in range(nsteps):
                i = turn[0] % nstreams
                turn[0] += 1
                if events is not None and not fake and not region:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(streams[i])
                    launch_own(i)
                    e1.record(streams[i])
                    events.append((e0, e1))
                else:
                    launch_own(i)
            if region:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(streams[0])
                events.append((e0, e1, nsteps))
            return
        limit = nsteps * len(units)
        while True:
            i = turn[0] % nstreams
            slot_wait(i)
            if bands_mode:
                # guided self-scheduling: a launch's efficiency grows with its size (a band of a deep zoom cannot be
                # shorter than its slowest block: 512-row bands of cfg3 run at 0.81 of the whole image's rate, 128-row
                # bands at 0.66), so a rank takes remaining / (2 N) consecutive bands of one image as ONE window
                t, k = cursor.next_guided(limit, 2 * pullers, period=len(units))
                if k == 0:
                    break
                first, last = units[t % len(units)], units[t % len(units) + k - 1]
                unit = Band(first.index, first.row0, last.row0 + last.nrows - first.row0)
            else:
                t, k = cursor.next(), 1
                if t >= limit:
                    break
                unit = units[t % len(units)]
            turn[0] += 1
            if events is not None:
                my_tickets.extend(range(t, t + k))
                launches[0] += 1
            launch_unit(i, unit)

    def census():
        """--shard queue, untimed: one pass over the tile set through the same cursor; every rank measures the
        pixel-iterations of the tiles it drew from the tiles' own output, and the per-tile figures are gathered:
        the work of a step is then known exactly without touching the timed region."""
        mine = {}
        while True:
            t = cursor.next()
            if t >= ntiles:
                break
            mine[t] = unit_stats(t)
        per_tile = {}
        for g in gather(mine):
            per_tile.update(g)
        assert sorted(per_tile) == list(range(ntiles)), "census: a tile was not measured"
        return per_tile

    per_tile = None
    if queue_mode:
        per_tile = census()
        # --queue-order longest: hand the tiles of a step out longest first (by the census' pixel-iterations; every rank holds the same table):
        # the last tickets of the run are then the cheapest tiles, so the ranks finish together -- the order a
        # Distributer hands tiles out in is the server's choice (Distributer.cs:335-353 walks its own list)
        if args.queue_order == "longest":
            units = sorted(units, key=lambda u: (-per_tile[u][0], u))
        barrier()
        if rank == 0:
            cursor.reset(0)
        barrier()
    smi = SmiSampler(gpu_index) if (args.full and not fake and rank == 0) else None
    # (sampled HERE, before the ramp, not between the warm-up and the timed region: the two SMI reads take ~2 ms, and a 2 ms idle
    # gap costs the next twenty launches 5-10 % -- scripts/burst_probe.py, profiles/r06/burst_probe_0.txt)
    smi_before = smi.sample() if smi else None
    if not fake:   # clock pre-conditioning (untimed, see --ramp-ms): every rank, its own GPU
        ramp_clock()
    run_steps(args.warmup if own_mode else max(args.warmup, 1))
    sync()
    barrier()
    if not own_mode:
        if rank == 0:
            cursor.reset(0)
        barrier()
    events = []
    t0 = time.perf_counter()
    run_steps(args.steps, events)
    host_submit_s = time.perf_counter() - t0     # the host's share: K launches enqueued, nothing waited for
    sync()
    my_finish = time.perf_counter() - t0
    barrier()
    elapsed = time.perf_counter() - t0
    smi_after = smi.sample() if smi else None     # (after the clock has been read: the SMI calls take milliseconds)
    # (units kernel, MBK_OPT_XCD_BALANCE: what share of a tile's heavy blocks every XCD was getting when the region ended)
    xcd_after_timed = dev.xcd_shares() if not fake and hasattr(dev, "xcd_shares") else None
    dumped = None
    if args.dump_outputs and rank == 0:   # (own mode on the GPU, checked before any work): the buffers of the last timed launch
        last = (turn[0] - 1) % nstreams
        outs = [("counts", d_counts_all[last], "float32")]          # int32 escape indices < 2^24: exact in float32
        if smooth:
            outs.append(("nu", d_smooth_all[last], "float64"))
        if d_bytes_all:
            outs.append(("bytes", d_bytes_all[last], "float32"))
        dumped = dump_outputs(args.dump_outputs, outs, npix)

    never = 0
    verified = None
    if queue_mode:
        iters_per_step = sum(v[0] for v in per_tile.values())
        never = sum(v[1] for v in per_tile.values())
        kernel_ms = [elapsed / args.steps * 1e3]
        kernel_ms_region = None
    elif fake:
        iters_per_step = 10 ** 9
        kernel_ms = [elapsed / args.steps * 1e3] * args.steps
        kernel_ms_region = None
    else:
        if bands_mode:      # work per step = the whole image, measured once (untimed) on every rank's own GPU
            launch_own(0)
            sync()
        st = dev.reduce_counts(d_counts_all[0].data_ptr(), npix, mrd, stream=streams[0].cuda_stream)
        iters_per_step, never = st.pixel_iterations, st.never_pixels
        if args.full and own_mode and rank == 0 and args.workload in golden_outputs():
            # the buffer the LAST TIMED launch wrote, against the CPU oracle's hash (VERDICT r4 missing 3)
            try:
                verified = verify_output(args.workload, d_counts_all[(turn[0] - 1) % nstreams], iters_per_step, never, view, mrd, args.precision)
            except Exception as e:   # noqa: BLE001 -- reported, must not cost the headline
                verified = {"verified": None, "why": repr(e)}
        region_events = bool(events) and len(events[0]) == 3
        if region_events:   # one pair around the K launches: the average; then (--full) an untimed pass with a pair per launch
            kernel_ms_region = events[0][0].elapsed_time(events[0][1]) / events[0][2]
            per_launch = []
            if args.full:
                saved, args.launch_events = args.launch_events, "per-launch"
                ramp_clock()     # (the GPU idled through the hash above)
                run_steps(max(min(args.steps, 64), 32), per_launch)
                sync()
                args.launch_events = saved
            kernel_ms = [a.elapsed_time(b) for a, b in per_launch]
        else:
            kernel_ms_region = None
            kernel_ms = [a.elapsed_time(b) for a, b in events] if events else [elapsed / args.steps * 1e3]

    # N > 1, strong-scaling modes: the SAME job on ONE GPU, timed in this very run.  N = 1 defaults
    # to one tile per step (`--shard own`: the contract's headline), N > 1 to the tile queue, whose single-GPU rate is
    # ~1.07x the headline's (finer pitch, more coherent blocks) -- so value(N) / value(1) across the two commands would
    # overstate the speed-up.  Here rank 0 pulls every ticket of the same steps from the same cursor, alone, while the
    # other ranks sit in a barrier (untimed for them); `single_gpu_same_job` in the line then gives the denominator
    # that belongs to `value`.  Errors are caught: this leg must not cost the headline (the barriers are unconditional).
    solo = None
    if world > 1 and not own_mode and not args.no_solo:
        barrier()
        if rank == 0:
            cursor.reset(0)
            try:
                run_steps(1, pullers=1)            # untimed: the GPU has idled through the barrier
                sync()
                cursor.reset(0)
                ts = time.perf_counter()
                run_steps(args.steps, pullers=1)
                sync()
                solo = time.perf_counter() - ts
            except Exception as e:   # noqa: BLE001 -- reported in the line, not swallowed
                solo = repr(e)
        barrier()

    # second leg (own mode, fp64/fp32 count kernels): the same K steps with the library's default cycle test.
    # A failure here must not cost the headline: errors are caught (the barriers stay unconditional, so the ranks
    # stay in step) and reported in config.cycle_leg_error instead of the cycle_detection object.
    cyc_leg, cyc_err, cyc_verified = None, None, None
    second_leg = args.full and not fake and own_mode and "cycle_detect" not in options and args.kernel in ("default", "group", "scan")
    cyc_steps, cyc_submit_s, cyc_event_ms = args.steps, None, None
    if second_leg:
        ce0, ce1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            dev.set_option("cycle_detect", 1)
            ramp_clock()
            ce0.record(streams[0])
            run_steps(max(args.warmup, 2))
            ce1.record(streams[0])
            sync()
            if world == 1 and nstreams == 1:   # at least MIN_LEG_MS of device time (N > 1: every rank times the same K steps)
                cyc_steps = max(args.steps, int(-(-MIN_LEG_MS // max(ce0.elapsed_time(ce1) / max(args.warmup, 2), 1e-3))))
        except Exception as e:   # noqa: BLE001 -- reported, not swallowed
            cyc_err = repr(e)
        barrier()
        t1 = time.perf_counter()
        try:
            if cyc_err is None:
                ce0.record(streams[0])
                run_steps(cyc_steps)
                cyc_submit_s = time.perf_counter() - t1
                ce1.record(streams[0])
                sync()
                if nstreams == 1:
                    cyc_event_ms = ce0.elapsed_time(ce1) / cyc_steps
        except Exception as e:   # noqa: BLE001
            cyc_err = repr(e)
        barrier()
        cyc_elapsed = time.perf_counter() - t1
        try:
            if cyc_err is None:
                st2 = dev.reduce_counts(d_counts_all[0].data_ptr(), npix, mrd, stream=streams[0].cuda_stream)
                cyc_leg = (cyc_elapsed, st2.pixel_iterations == iters_per_step and st2.never_pixels == never)
                if rank == 0 and verified is not None and verified.get("verified") is not None:
                    cyc_verified = verify_output(args.workload, d_counts_all[(turn[0] - 1) % nstreams], st2.pixel_iterations, st2.never_pixels,
                                                 view, mrd, args.precision)
            dev.set_option("cycle_detect", 0)
        except Exception as e:   # noqa: BLE001
            cyc_err, cyc_leg = repr(e), None

    once = None
    per_rank_units = None
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if backend == "gloo" else f"cuda:{gpu_index}")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed_max = float(t.item())
        if second_leg:
            # every rank takes part (elapsed < 0 marks a rank whose leg failed: then no rank reports the leg)
            t = torch.tensor([cyc_leg[0] if cyc_leg else -1.0, -(cyc_leg[0] if cyc_leg else -1.0)], dtype=torch.float64,
                             device="cpu" if backend == "gloo" else f"cuda:{gpu_index}")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)      # [max elapsed, -min elapsed]
            if cyc_leg is not None and -float(t[1].item()) >= 0.0:
                cyc_leg = (float(t[0].item()), cyc_leg[1])
            else:
                cyc_leg = None
    else:
        elapsed_max = elapsed
    ranks_seen = gather(me)
    gather_launches = gather(launches[0])
    finish_ms = [round(x * 1e3, 3) for x in gather(my_finish)]
    if not own_mode:
        gathered = gather(my_tickets)
        allt = sorted(x for g in gathered for x in g)
        once = allt == list(range(args.steps * len(units)))
        per_rank_units = [len(g) for g in gathered]
    # weak scaling: every rank did the same tile; strong scaling: the ranks shared the work of every step
    iters_all = float(iters_per_step) * (world if own_mode else 1)

    if rank == 0:
        if kernel_ms_region is not None:   # events around the whole timed region / K (what the roofline is priced on)
            avg_kernel_s = kernel_ms_region / 1e3
        else:
            avg_kernel_s = sum(kernel_ms) / len(kernel_ms) / 1e3
        if not own_mode:      # per-GPU average time per step, idle time included
            avg_kernel_s = elapsed_max / args.steps
        cus, mhz = device_info["compute_units"], device_info["clock_mhz"]
        lanes_per_clk = 16 if args.precision == "f64" else 32  # per SIMD: fp64 16, fp32 32 (SIMD-32)
        peak_lane_ops = cus * 4 * lanes_per_clk * mhz * 1e6    # VALU lane-ops/s of that type
        peak_tflops = peak_lane_ops * 2 / 1e12                 # FMA = 2 flop -> 78.6 (fp64) / 157.3 (fp32)
        per_gpu_iters = iters_per_step / (1 if own_mode else world)
        achieved_tflops = FLOPS_PER_PIXEL_ITER * per_gpu_iters / avg_kernel_s / 1e12
        slots = VALU_SLOTS_PER_PIXEL_ITER.get(args.kernel, 8.0)
        if args.kernel in ("default", "scan", "group") and options.get("group_steps", 16) != 16:
            slots = {8: 6.25, 32: 6.0625 if args.kernel != "scan" else 6.125}.get(options["group_steps"], 6.5)
        if options.get("cycle_detect", 0) and args.kernel in ("default", "scan", "group") and options.get("group_steps", 16) != 4:
            slots += 0.125     # two bitwise state compares per 16 steps
        launches_per_step = ntiles if queue_mode else 1
        out_bytes = npix * (12 if smooth else 4) * launches_per_step // (1 if own_mode else world)
        traffic, traffic_source = pmc_traffic(args.workload, args.kernel) if args.precision == "f64" and not options and own_mode else (None, None)
        metric = "G pixel-iterations/s on 4096^2 tile, max_iter=1000 fp64"
        if own_mode:
            how = "one tile per GPU per step"
        elif queue_mode:
            how = (f"one step = {ntiles} tiles of {width}x{height} ({args.grid}x{args.grid} grid over the same region at "
                   f"{args.grid}x finer pitch), pulled by all ranks from one shared cursor, {nstreams} in flight per GPU")
        else:
            how = (f"one image per step cut into {len(bands)} row bands of {band_rows} rows pulled from a shared cursor, "
                   "several consecutive bands per launch while many are left (guided self-scheduling)")
        cfg = {"workload": f"{args.workload}: {desc}; {how}, int32 counts written to resident HBM",
               "kernel": args.kernel, "options": options, "outputs": args.outputs,
               "cycle_test": ("on (--opt)" if options.get("cycle_detect", 0) else
                              "off for value and roofline: every iteration the reference runs is executed" +
                              ("; the library default (on) is timed in this run: see cycle_detection" if cyc_leg else "")),
               "pixels_per_step": npix * (world if own_mode else launches_per_step),
               "pixel_iterations_per_step_per_gpu": per_gpu_iters,
               "never_escaped_pixels": never, "parallelism": f"{world} independent work queue(s), no collective"
               if own_mode else f"{world} rank(s) pulling from one shared cursor, no collective",
               "streams_per_gpu": nstreams, "shard": args.shard, "control_backend": backend,
               "clock_ramp_ms": args.ramp_ms if not fake else 0.0,
               "fake_backend": fake, "device": device_info.get("name"), "compute_units": cus, "clock_mhz": mhz,
               "cycle_leg_error": cyc_err,
               "host_submit_us_per_launch": host_submit_s / max(1, args.steps) * 1e6 if own_mode else None,
               "versions": box_versions(torch, smi) if smi else None,
               "smi_around_timed_region": ({"before_ramp": {"power_W": smi_before[1], "sclk_MHz": smi_before[2]} if smi_before else None,
                                            "after": {"power_W": smi_after[1], "sclk_MHz": smi_after[2]} if smi_after else None,
                                            "power_cap_W": smi.cap_w} if smi else None),
               "occupancy_api_wg_per_cu": device_info.get("scan_occupancy"),
               "xcd_balance": f"{options['xcd_balance']} (--opt)" if "xcd_balance" in options else "0 (library default)",
               "xcd_shares": xcd_after_timed,
               "launcher": "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else
                           ("bench.py self-launch" if "MBK_BENCH_RUN_ID" in os.environ else "single process"),
               "oversubscribed": bool(args.oversubscribe),
               "ranks_seen": ranks_seen,
               "distinct_gpus": len({(r["host"], r["pci_bus_id"], r["gpu_index"]) for r in ranks_seen}),
               "rank_finish_ms": finish_ms}
        if bands_mode:
            cfg.update({"bands_per_image": len(bands), "band_rows": band_rows, "bands_exactly_once": once,
                        "bands_per_rank": per_rank_units, "launches_per_rank": gather_launches,
                        "band_scheduling": "guided: remaining / (2 N) consecutive bands of one image per launch"})
        if queue_mode:
            tile_iters = [per_tile[k][0] for k in range(ntiles)]
            cfg.update({"tiles_per_step": ntiles, "grid": args.grid, "tiles_exactly_once": once,
                        "tiles_per_rank": per_rank_units,
                        "tile_order": "longest first within a step (census)" if args.queue_order == "longest" else
                                      "image order (the server's walk of its own list)",
                        "tile_pixel_iterations_min_max": [min(tile_iters), max(tile_iters)]})
        rec = {
            "metric": metric,
            "value": iters_all * args.steps / elapsed_max / 1e9,
            "unit": "G pixel-iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed_max / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak" if own_mode else "strong",
            "vs_baseline": None,
            "dtype": args.precision,
            "data": "synthetic (coordinates generated in-kernel from the view origin and stride; no RNG)",
            "config": cfg,
            "roofline": {
                "bound": "fp64_valu" if args.precision == "f64" else "fp32_valu",
                "achieved": achieved_tflops,
                "peak": peak_tflops,
                "unit": "TFLOP/s",
                "frac": achieved_tflops / peak_tflops,
                "traffic": traffic,
                "traffic_source": traffic_source,
                "basis": ("one pair of HIP events on the launch stream around the K launches of the timed region, elapsed / K "
                          "(gaps between launches included); median / min / kernel_ms_avg_per_launch_pass: "
                          + (f"an untimed pass of {len(kernel_ms)} launches with a pair of events per launch" if kernel_ms
                             else "not measured (--full runs a pass with a pair of events per launch)")
                          if kernel_ms_region is not None else "HIP events around each launch on its stream") if own_mode
                         else "whole-job wall time per step per GPU (idle time included)",
                "kernel_ms_avg_per_launch_pass": sum(kernel_ms) / len(kernel_ms) if kernel_ms_region is not None and kernel_ms else None,
                "kernel_ms_avg": avg_kernel_s * 1e3,
                "kernel_ms_median": (sorted(kernel_ms)[len(kernel_ms) // 2] if kernel_ms else None) if own_mode else avg_kernel_s * 1e3,
                "kernel_ms_min": min(kernel_ms) if kernel_ms else None,
                "flops_per_pixel_iteration": FLOPS_PER_PIXEL_ITER,
                "valu_slots_per_pixel_iteration": slots,
                # with the cycle test in the headline (--opt cycle_detect=1) fewer steps are executed than the
                # reference's count says, so the executed-issue figures cannot be derived from the output
                "parity_ceiling_frac": None if options.get("cycle_detect", 0) else FLOPS_PER_PIXEL_ITER / (2.0 * slots),
                "valu_slot_util": None if options.get("cycle_detect", 0) else slots * per_gpu_iters / avg_kernel_s / peak_lane_ops,
                "algorithmic_hbm_bytes_per_launch": npix * (12 if smooth else 4),
                "hbm_GBps": out_bytes / avg_kernel_s / 1e9,
            },
        }
        if verified is not None:
            rec["output_verified"] = dict(verified, what="sha256 of the int32 counts the last timed launch wrote (one D2H after the timed "
                                                         "region) and the two totals, against the CPU oracle's")
        if isinstance(solo, float):
            solo_value = iters_all * args.steps / solo / 1e9
            rec["single_gpu_same_job"] = {
                "what": "the same job (same tiles / bands, same steps, same cursor, same streams in flight) pulled by rank 0 "
                        "alone on its one GPU right after the timed region, the other ranks waiting in a barrier: the N = 1 "
                        "point that belongs to `value` (the plain `--gpus 1` command measures one tile per step instead)",
                "value": solo_value, "unit": "G pixel-iterations/s", "ms_per_step": solo / args.steps * 1e3,
                "steps": args.steps, "gpu": me.get("pci_bus_id")}
            rec["speedup_same_job"] = rec["value"] / solo_value
            rec["efficiency_same_job"] = rec["value"] / (world * solo_value)
        elif solo is not None:
            rec["single_gpu_same_job"] = {"error": solo}
        if cyc_leg is not None:
            rec["cycle_detection"] = {
                "what": "same workload and steps with MBK_OPT_CYCLE_DETECT=1 (library default): pixels whose (zr, zi) bit "
                        "pattern repeats are retired as 'never escapes' -- identical counts, fewer executed steps; value "
                        "counts the reference's iterations, not the executed ones",
                "value": iters_all * cyc_steps / cyc_leg[0] / 1e9,
                "unit": "G pixel-iterations/s (reference-equivalent)",
                "ms_per_step": cyc_leg[0] / cyc_steps * 1e3,
                "steps": args.steps, "steps_run": cyc_steps, "clock_ramp_ms": args.ramp_ms,
                "kernel_ms_avg": cyc_event_ms,
                "basis": "ms_per_step: wall clock around steps_run launches and the final synchronise; kernel_ms_avg: one pair of HIP "
                         "events on the launch stream around the same launches, elapsed / steps_run",
                "host_submit_us_per_launch": cyc_submit_s / cyc_steps * 1e6 if cyc_submit_s is not None else None,
                "speedup_vs_strict": (elapsed_max / args.steps) / (cyc_leg[0] / cyc_steps),
                "same_pixel_iterations_and_never_count": bool(cyc_leg[1]),
                "output_verified": cyc_verified,
            }
        if dumped is not None:
            rec["outputs_dumped"] = dumped
        if (args.full and world == 1 and own_mode and not fake and not args.no_extras and args.workload == "cfg2" and not smooth
                and args.precision == "f64" and args.kernel == "default" and not options):
            # beside the headline (never in `value`): the end-to-end tile rate, and the N > 1 default job on this GPU
            # -- `sustained`: the headline's launches back to back for >= SUSTAINED_S, clock / power sampled through librocm_smi64
            # (VERDICT r5 missing 3: every other timed region of this line is 10-100 ms on a board that runs at its power cap)
            try:
                dev.set_option("cycle_detect", 0)
                ramp_clock()
                n_sus = max(args.steps, int(SUSTAINED_S * 1e3 / max(rec["ms_per_step"], 1e-3)) + 1)
                se0, se1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stop_trace = smi.trace(0.01) if smi else (lambda: [])
                ts = time.perf_counter()
                se0.record(streams[0])
                for _ in range(n_sus):
                    launch_own(0)
                sus_submit = time.perf_counter() - ts
                se1.record(streams[0])
                sync()
                te = time.perf_counter()
                rows = [r for r in stop_trace() if ts <= r[0] <= te]

                def at(frac):
                    if not rows:
                        return None
                    r = rows[min(len(rows) - 1, int(frac * len(rows)))]
                    return {"t_ms": round((r[0] - ts) * 1e3, 1), "power_W": r[1], "sclk_MHz": r[2]}
                sus_ms = se0.elapsed_time(se1) / n_sus
                rec["sustained"] = {
                    "what": f"the headline's workload and options (cycle test off, library defaults), {n_sus} launches back to back on one "
                            f"stream = at least {SUSTAINED_S:.0f} s of device time; board power and shader clock sampled through "
                            "librocm_smi64 while it runs (the SMI figures are the firmware's own moving averages)",
                    "steps_run": n_sus, "seconds": te - ts, "value": iters_per_step * n_sus / (te - ts) / 1e9, "unit": "G pixel-iterations/s",
                    "ms_per_step": (te - ts) / n_sus * 1e3, "kernel_ms_avg": sus_ms,
                    "roofline_frac": FLOPS_PER_PIXEL_ITER * iters_per_step / (sus_ms / 1e3) / 1e12 / peak_tflops,
                    "ratio_to_headline_value": (iters_per_step * n_sus / (te - ts) / 1e9) / rec["value"],
                    "host_submit_us_per_launch": sus_submit / n_sus * 1e6,
                    "power_cap_W": smi.cap_w if smi else None, "smi_samples": len(rows),
                    "start": at(0.02), "middle": at(0.5), "end": at(0.98),
                    "sclk_MHz_min_max": [min(r[2] for r in rows if r[2]), max(r[2] for r in rows if r[2])] if any(r[2] for r in rows) else None,
                    "power_W_max": max((r[1] for r in rows if r[1]), default=None),
                }
            except Exception as e:   # noqa: BLE001
                rec["sustained"] = {"error": repr(e)}
            # -- `xcd_balance_opt_in`: the headline's K steps with MBK_OPT_XCD_BALANCE = 1 (rounds 4-5 measured `value` this way)
            try:
                dev.set_option("xcd_balance", 1)
                ramp_clock()
                run_steps(max(args.warmup, 8))     # the shares are learned from launches on the stream: the ramp's and these
                sync()
                n_x = max(args.steps, int(-(-MIN_LEG_MS // max(rec["ms_per_step"], 1e-3))))
                xe0, xe1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                tx = time.perf_counter()
                xe0.record(streams[0])
                run_steps(n_x)
                xe1.record(streams[0])
                sync()
                dx = time.perf_counter() - tx
                rec["xcd_balance_opt_in"] = {
                    "what": "the headline's workload with MBK_OPT_XCD_BALANCE = 1 (opt-in; library default 0): uneven shares of the heavy "
                            "list per XCD, learned from the time stamps of earlier solitary launches on the stream -- not part of `value`",
                    "value": iters_per_step * n_x / dx / 1e9, "unit": "G pixel-iterations/s", "ms_per_step": dx / n_x * 1e3,
                    "kernel_ms_avg": xe0.elapsed_time(xe1) / n_x, "steps_run": n_x, "ratio_to_headline_value": (iters_per_step * n_x / dx / 1e9) / rec["value"],
                    "xcd_shares": dev.xcd_shares()}
            except Exception as e:   # noqa: BLE001
                rec["xcd_balance_opt_in"] = {"error": repr(e)}
            finally:
                dev.set_option("xcd_balance", options.get("xcd_balance", 0))
            try:   # the same strict steps with TWO launches in flight (two streams): what a two-slot worker context does
                s2 = torch.cuda.Stream()
                buf2 = torch.empty(npix, dtype=torch.int32, device=f"cuda:{gpu_index}")

                def launch2(k):
                    dev.launch_view(view, mrd, d_counts=(d_counts_all[0] if k % 2 == 0 else buf2).data_ptr(),
                                    stream=(streams[0] if k % 2 == 0 else s2).cuda_stream, kernel=args.kernel,
                                    precision=args.precision)
                ramp_clock()
                for k in range(max(args.warmup, 4)):
                    launch2(k)
                sync()
                n_2 = max(args.steps, int(-(-MIN_LEG_MS // max(rec["ms_per_step"], 1e-3))))
                n_2 += n_2 % 2
                t2 = time.perf_counter()
                for k in range(n_2):
                    launch2(k)
                sync()
                dt2 = time.perf_counter() - t2
                rec["two_streams"] = {"what": "the headline's launches (cycle test off) issued alternately on two streams: the tail of one "
                                              "launch overlaps the head of the next; per-launch events no longer isolate a kernel, so "
                                              "this is a wall-clock rate only",
                                      "value": iters_per_step * n_2 / dt2 / 1e9, "unit": "G pixel-iterations/s", "steps_run": n_2,
                                      "ms_per_step": dt2 / n_2 * 1e3, "ratio_to_headline_value": (iters_per_step * n_2 / dt2 / 1e9) / rec["value"]}
            except Exception as e:   # noqa: BLE001
                rec["two_streams"] = {"error": repr(e)}
            try:
                dev.set_option("cycle_detect", 1)
                rec["end_to_end"] = end_to_end(dev)
            except Exception as e:   # noqa: BLE001 -- reported, must not cost the headline
                rec["end_to_end"] = {"error": repr(e)}
            finally:
                dev.set_option("cycle_detect", options.get("cycle_detect", 0))
            rec["queue_job"] = queue_job_single(args, rec["value"])
            try:
                dev.set_option("cycle_detect", 0)
                rec["configs"] = extra_configs(dev, torch, gpu_index, device_info, ramp_ms=args.ramp_ms if args.ramp_ms > 0 else 0.0)
            except Exception as e:   # noqa: BLE001
                rec["configs"] = {"error": repr(e)}
        if args.full and world == 1 and not args.no_cpu_baseline and not fake:
            rec["cpu_baseline"] = cpu_baseline(args.workload, workload, args.precision)
        elif args.full and world == 1 and fake:
            rec["cpu_baseline"] = None
        print(json.dumps(rec), flush=True)

    if cursor is not None:
        barrier()
        cursor.close()
    if world > 1:
        dist.destroy_process_group()
    if dev is not None:
        dev.close()
    if smi is not None:
        smi.close()


def queue_job_single(args, headline_value):
    """The N > 1 default job (--shard queue) on ONE GPU, in a process of its own: the same-mode N = 1 point of the
    scaling curve (value(N) / (N x this) is the efficiency of the queue; `value` of the headline is a single tile
    per step, whose rate differs by the tiles' pitch)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--shard", "queue", "--full", "--no-cpu-baseline", "--no-extras",
           "--workload", args.workload, "--kernel", args.kernel, "--grid", str(args.grid), "--steps", "3", "--warmup", "1",
           "--queue-order", args.queue_order]
    for item in args.opt:
        cmd += ["--opt", item]
    try:
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        return {"what": "the default N > 1 job (--shard queue) on this one GPU: " + rec["config"]["workload"],
                "value": rec["value"], "unit": rec["unit"], "ms_per_step": rec["ms_per_step"], "steps": rec["steps"],
                "tiles_per_step": rec["config"]["tiles_per_step"], "tiles_exactly_once": rec["config"]["tiles_exactly_once"],
                "ratio_to_headline_value": rec["value"] / headline_value if headline_value else None}
    except Exception as e:   # noqa: BLE001
        return {"error": repr(e)}


if __name__ == "__main__":
    main()
