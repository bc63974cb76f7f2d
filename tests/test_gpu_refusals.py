"""What the view calls of the C ABI refuse, call by call: the status, the exact text (device._error_text) and outputs left as
they were.  One table of (kind of view, call, what differs from a served call, message) over the count calls of the deep,
extended-range and Julia views, the renders and histograms of all four kinds, and the density calls.  Nothing is launched."""
import ctypes as C

import numpy as np
import pytest

from distributedmandelbrot_amd import DeepOrbit
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _error_text

pytestmark = pytest.mark.gpu

MRD, N = 50, 16
BOTH = L.MBK_WANT_COUNTS | L.MBK_WANT_BYTES
F32, BLA, GROUP, SIMPLE, SCAN = L.MBK_PRECISION_F32, L.MBK_DEEP_BLA, L.MBK_KERNEL_GROUP, L.MBK_KERNEL_SIMPLE, L.MBK_KERNEL_SCAN
PREFIX = {"plain": "mbk_view_", "julia": "mbk_julia_view_", "deep": "mbk_deep_view_", "wide": "mbk_deep_xview_"}
NAME = {"launch": "launch", "compute": "compute", "submit": "submit", "render_launch": "render_launch",
        "render_compute": "render_compute", "eq_launch": "render_equalized_launch", "eq_compute": "render_equalized_compute",
        "hist_launch": "histogram_launch", "hist_compute": "histogram_compute", "density_launch": "density_launch",
        "density_compute": "density_compute"}
VIEW = {"plain": dict(start_r=-1.6, start_i=-1.2, range_r=3.2, range_i=2.4), "julia": dict(start_r=-1.6, start_i=-1.2, range_r=3.2, range_i=2.4),
        "deep": dict(range_r=1e-20, range_i=1e-20), "wide": dict(range_r=1.0, range_i=1.0, exp2=-50)}
GEOMETRY = dict(width=N, height=N, col0=0, row0=0, ncols=N, nrows=N)
STRUCT = {"plain": L.mbk_view, "julia": L.mbk_view, "deep": L.mbk_deep_view, "wide": L.mbk_deep_xview}

# ---- the messages -------------------------------------------------------------------------------------------------------
INT32 = "mrd must fit int32 (calc_mb_value returns int32)"
NO_QUANT = "mrd == 0 has no quantised form (division by zero)"
COORD = "view coordinates must be finite and |x| <= 2^500"
TOO_DEEP = "mrd exceeds the mrd the reference orbit was computed for"
SELECTOR = "unknown MBK_KERNEL_* selector"
JULIA_KERNELS = "Julia views are implemented by MBK_KERNEL_DEFAULT / _ASM / _GROUP only"
RANGE = {"deep": "deep view ranges must be finite and lie in [2^-960, 4]",
         "wide": "extended-range deep view ranges must be finite and lie in [2^-64, 4]", "plain": COORD, "julia": COORD}
EXP2 = "extended-range deep view exp2 must lie in [-8192, 0]"
COUNT_FLAGS = {"deep": "deep views take MBK_WANT_COUNTS / MBK_WANT_BYTES / MBK_DEEP_BLA only (no kernel selection, no fp32)",
               "wide": "extended-range deep views take MBK_WANT_COUNTS / MBK_WANT_BYTES only (no kernel selection, no fp32)",
               "julia": "Julia views take MBK_WANT_COUNTS / MBK_WANT_BYTES and kernel selection only (no fp32, no MBK_LAZY_UNIFORM)"}
WIDE_BLA = "MBK_DEEP_BLA is not implemented for extended-range deep views"
NO_OUTPUT = {"launch": "flags and d_smooth select no output", "compute": "flags and h_smooth select no output",
             "submit": "flags select no output"}
RENDER_FLAGS = {"plain": "render flags carry kernel selection (and MBK_PRECISION_F32) only",
                "julia": "Julia render flags carry kernel selection only",
                "deep": "deep renders take MBK_DEEP_BLA only (no kernel selection, no fp32)",
                "wide": "extended-range deep renders take no flags (no MBK_DEEP_BLA, no kernel selection, no fp32)"}
HIST_FLAGS = {"plain": "histogram flags carry kernel selection and MBK_PRECISION_F32 only",
              "julia": "Julia histogram flags carry kernel selection only",
              "deep": "deep histograms take MBK_DEEP_BLA only (no kernel selection, no fp32)",
              "wide": "extended-range deep histograms take no flags (no MBK_DEEP_BLA, no kernel selection, no fp32)"}
# a flag each kind's renders and histograms refuse
BAD_FLAG = {"plain": L.MBK_WANT_COUNTS, "julia": F32, "deep": GROUP, "wide": BLA}
HIST_MRD = "mrd must lie in [1, MBK_HISTOGRAM_MAX_MRD]"
REL_PLAIN = "MBK_RENDER_DISTANCE_REL is implemented for deep views only (plain views: MBK_RENDER_DISTANCE)"
NO_WIDE_DISTANCE = "distance estimates are not implemented for extended-range deep views"
SMOOTH_KERNELS = "smooth colouring and MBK_PRECISION_F32 are implemented by the scan / asm / group kernels only"


def _cases():
    out = []

    def add(kind, ops, message, **change):
        out.extend((kind, op, change, message) for op in ops)

    for kind in ("deep", "wide", "julia", "plain"):
        counts = () if kind == "plain" else ("launch", "compute", "submit")
        renders = ("render_launch", "render_compute", "eq_launch", "eq_compute")
        hists = ("hist_launch", "hist_compute")
        density = ("density_launch", "density_compute") if kind == "plain" else ()
        every = counts + renders + hists + density
        # the view and its window
        add(kind, every, "view is NULL", view=None)
        add(kind, every, "empty view", width=0, height=0, ncols=0, nrows=0)
        add(kind, every, "empty window", ncols=0)
        add(kind, every, "empty window", nrows=0)
        add(kind, every, "window exceeds the view", col0=10, ncols=7)
        add(kind, every, "window exceeds the view", row0=N, nrows=1)
        add(kind, counts + hists + density, "empty view", width=0)
        add(kind, renders, "window exceeds the view", width=0)                    # a render looks at the output window first
        add(kind, every, RANGE[kind], range_r=float("nan"))
        add(kind, every, RANGE[kind], range_i=float("inf"))
        if kind in ("deep", "wide"):
            add(kind, every, "orbit is NULL", orbit=None)
            add(kind, counts, "orbit is NULL", orbit=None, view=None)
            add(kind, renders + hists, "view is NULL", orbit=None, view=None)
            add(kind, every, RANGE[kind], range_r=2.0 ** (-961 if kind == "deep" else -65))
            add(kind, every, RANGE[kind], range_i=4.5)
            add(kind, every, TOO_DEEP, mrd=101)
            add(kind, counts, "orbit is NULL", orbit=None, range_r=float("nan"))
            add(kind, counts, "empty view", width=0, mrd=101)
        if kind == "wide":
            add(kind, every, EXP2, exp2=1)
            add(kind, every, EXP2, exp2=-8193)
            add(kind, counts, WIDE_BLA, flags=BOTH | BLA)
            add(kind, counts, WIDE_BLA, flags=BOTH | BLA, exp2=1)                 # two faults: the flag is looked at first
            add(kind, renders, RENDER_FLAGS[kind], flags=BLA, exp2=1)
            add(kind, hists, HIST_FLAGS[kind], flags=BLA, exp2=1)
        if kind in ("plain", "julia"):
            add(kind, counts + renders + density, INT32, mrd=1 << 31)
            add(kind, hists, HIST_MRD, mrd=1 << 31)
        if kind == "julia":
            add(kind, every, "the Julia parameter must be finite", c=(float("nan"), 0.0))
            add(kind, every, "the Julia parameter must be finite", c=(0.0, float("inf")))
            add(kind, counts, JULIA_KERNELS, flags=BOTH | SCAN)
            add(kind, renders + hists, JULIA_KERNELS, flags=SCAN)
            add(kind, counts, COUNT_FLAGS[kind], flags=BOTH | F32, view=None)
            add(kind, counts, JULIA_KERNELS, flags=BOTH | SIMPLE, c=(float("nan"), 0.0))
        # the count calls' own rules
        add(kind, counts, "ctx is NULL", ctx=None)
        add(kind, counts, "ctx is NULL", ctx=None, view=None)
        add(kind, counts, NO_QUANT, mrd=0)
        for op in counts:
            add(kind, (op,), COUNT_FLAGS[kind], flags=BOTH | (GROUP if kind != "julia" else F32))
            add(kind, (op,), COUNT_FLAGS[kind], flags=BOTH | L.MBK_LAZY_UNIFORM, ncols=0)      # two faults: bad flags, empty window
            add(kind, (op,), NO_OUTPUT[op], flags=0)
            add(kind, (op,), "MBK_WANT_COUNTS with NULL counts pointer", counts=None)
            add(kind, (op,), "MBK_WANT_BYTES with NULL bytes pointer", bytes=None)
            add(kind, (op,), "empty window", flags=0, ncols=0)
        add(kind, counts[2:], "slot out of range", slot=L.MBK_SLOTS)
        add(kind, counts[2:], "slot out of range", slot=-1)
        add(kind, counts[2:], "slot out of range", slot=L.MBK_SLOTS, view=None)           # two faults: bad slot, NULL view
        add(kind, counts[2:], "slot out of range", slot=-1, flags=0)
        # renders
        add(kind, renders, "ctx is NULL", ctx=None)
        add(kind, renders, "render spec is NULL", spec=None)
        add(kind, renders, "render spec is NULL", spec=None, view=None)
        add(kind, renders, "palette is NULL", palette=None)
        add(kind, renders, "output pointer is NULL", out=None)
        add(kind, renders, "output pointer is NULL", out=None, view=None)
        add(kind, renders, "supersample must be 1, 2, 3, 4 or 8", supersample=5)
        add(kind, renders, "supersample must be 1, 2, 3, 4 or 8", supersample=0, ncols=0)
        add(kind, renders[:2], "MBK_RENDER_EQUALIZED needs a table: use the equalized calls", source=L.MBK_RENDER_EQUALIZED)
        add(kind, renders[2:], "the equalized calls take MBK_RENDER_EQUALIZED only", source=L.MBK_RENDER_SMOOTH)
        add(kind, renders[:2], "unknown MBK_RENDER_* source", source=2)
        add(kind, renders[:2], "MBK_RENDER_BYTES takes a palette of 256 entries", source=L.MBK_RENDER_BYTES)
        add(kind, renders, "MBK_RENDER_SMOOTH / _EQUALIZED take a palette of 2 .. 65536 entries", palette_len=1)
        add(kind, renders, "scale must lie in (0, 2^20]", scale=0.0)
        add(kind, renders, "offset must lie in [-2^20, 2^20]", offset=float("nan"))
        add(kind, renders, "width or height times supersample does not fit 32 bits", width=1 << 31, supersample=2)
        add(kind, renders, RENDER_FLAGS[kind], flags=BAD_FLAG[kind])
        add(kind, renders, RENDER_FLAGS[kind], flags=BAD_FLAG[kind], ncols=0)            # two faults: bad flags, empty window
        add(kind, renders[:2], NO_QUANT, mrd=0, source=L.MBK_RENDER_BYTES, palette_len=256)
        add(kind, renders[2:], "equalisation table is NULL", lut=None)
        add(kind, renders[2:], "lut_len must equal mrd + 2", lut_len=MRD + 1)
        add(kind, renders[2:], "equalisation table entries must be finite and lie in [0, 1]", lut_entry=2.0)
        add(kind, renders[2:], "equalisation table entries must be finite and lie in [0, 1]", lut_entry=float("nan"))
        add(kind, renders[2:], "empty window", lut=None, ncols=0)
        add(kind, ("render_launch", "eq_launch"), "d_rgba must be 4-byte aligned", misalign=2)
        for source in (L.MBK_RENDER_DISTANCE, L.MBK_RENDER_DISTANCE_REL):
            rel = source == L.MBK_RENDER_DISTANCE_REL
            if kind == "wide":
                add(kind, renders[:2], NO_WIDE_DISTANCE, source=source)
                add(kind, renders[:2], NO_WIDE_DISTANCE, source=source, flags=BLA)
            elif kind == "deep" and not rel:
                add(kind, renders[:2], "MBK_RENDER_DISTANCE is implemented for plain views only (no deep renders)", source=source)
            elif kind == "deep":
                add(kind, renders[:2], "MBK_DEEP_BLA is not implemented for deep distance estimates", source=source, flags=BLA)
                add(kind, renders[:2], RENDER_FLAGS[kind], source=source, flags=BLA | GROUP)
            elif rel:
                add(kind, renders[:2], REL_PLAIN, source=source)
            elif kind == "julia":
                add(kind, renders[:2], "MBK_RENDER_DISTANCE is implemented for Mandelbrot views only (no Julia renders)", source=source)
            else:
                add(kind, renders[:2], SMOOTH_KERNELS, source=source, flags=SIMPLE)
                add(kind, renders[:2], "smooth colouring is implemented in binary64 only", source=source, flags=F32)
            add(kind, renders[:2], "MBK_RENDER_DISTANCE / _DISTANCE_REL take a palette of 2 .. 65536 entries", source=source, palette_len=1)
            add(kind, renders[:2], "scale must lie in (0, 2^80]", source=source, scale=float("inf"))
        # histograms
        add(kind, hists, "ctx is NULL", ctx=None)
        add(kind, hists, "histogram pointer is NULL", out=None)
        add(kind, hists, "histogram pointer is NULL", out=None, view=None)
        add(kind, hists, "view is NULL", view=None, mrd=0)
        add(kind, hists, HIST_MRD, mrd=0)
        add(kind, hists, HIST_MRD, mrd=L.MBK_HISTOGRAM_MAX_MRD + 1, flags=BAD_FLAG[kind])
        add(kind, hists, HIST_FLAGS[kind], flags=BAD_FLAG[kind])
        add(kind, hists, HIST_FLAGS[kind], flags=BAD_FLAG[kind], ncols=0)                # two faults: bad flags, empty window
        add(kind, ("hist_launch",), "d_hist must be 8-byte aligned", misalign=4)
        if kind == "deep":
            add(kind, renders + hists, TOO_DEEP, flags=BLA, mrd=101)
            add(kind, renders + hists, "empty window", flags=BLA, ncols=0)
        if kind == "plain":
            add(kind, renders + hists, SELECTOR, flags=0x600)
            add(kind, renders, SMOOTH_KERNELS, flags=SIMPLE)
            add(kind, renders, SMOOTH_KERNELS, flags=L.MBK_KERNEL_REFILL)
            add(kind, renders[:2], SMOOTH_KERNELS, flags=SIMPLE | F32, source=L.MBK_RENDER_BYTES, palette_len=256)
            add(kind, renders, "smooth colouring is implemented in binary64 only", flags=F32)
            add(kind, renders, "view coordinates must be finite and |x| <= 2^60 (fp32)", flags=F32, range_r=2.0 ** 70)
            add(kind, renders, INT32, flags=0x600, mrd=1 << 31)                          # two faults: mrd is looked at first
            add(kind, hists, "MBK_PRECISION_F32 is implemented by the scan / asm / group kernels only", flags=F32 | SIMPLE)
            add(kind, hists, "view coordinates must be finite and |x| <= 2^60 (fp32)", flags=F32, range_r=2.0 ** 70)
            add(kind, hists, "empty window", flags=0x600, ncols=0)
            # density
            add(kind, density, "NULL argument", ctx=None)
            add(kind, density, "NULL argument", out=None)
            add(kind, density, "NULL argument", out=None, view=None)
            add(kind, density, "density flags carry kernel selection only (no fp32, no MBK_LAZY_UNIFORM, no MBK_DEEP_BLA)", flags=F32)
            add(kind, density, "density flags carry kernel selection only (no fp32, no MBK_LAZY_UNIFORM, no MBK_DEEP_BLA)", flags=BLA, ncols=0)
            add(kind, density, SELECTOR, flags=0x600)
            add(kind, density, SELECTOR, flags=0x600, view=None)
            add(kind, density, "density views take their counts from the scan / asm / group kernels only", flags=SIMPLE)
            add(kind, density, "min_count must be at least 1 (a sample that never escapes deposits nothing)", min_count=0)
            add(kind, density, "max_count must be below mrd", max_count=MRD)
            add(kind, density, "min_count exceeds max_count", min_count=10, max_count=5)
            add(kind, density, "density target is NULL", target=None)
            add(kind, density, "min_count must be at least 1 (a sample that never escapes deposits nothing)", min_count=0, target=None)
            add(kind, density, "density target must hold 1 .. 2^28 cells", t_width=0)
            add(kind, density, "density target must hold 1 .. 2^28 cells", t_width=1 << 15, t_height=(1 << 13) + 1)
            add(kind, density, "density target start must be finite", t_start_r=float("nan"))
            add(kind, density, "density target ranges must be finite and > 0", t_range_i=0.0)
            add(kind, ("density_launch",), "d_density must be 4-byte aligned", misalign=2)
    return out


CASES = _cases()


def _id(case):
    kind, op, change, _ = case
    return f"{kind}-{op}-" + ",".join(change)


class Buffers:
    """Host and device outputs, filled once: a refused call leaves every one of them as it is."""

    def __init__(self):
        import torch
        self.torch = torch
        self.host = {"counts": np.full(N * N, -7, np.int32), "bytes": np.full(N * N, 0xA5, np.uint8), "smooth": np.full(N * N, -7.0),
                     "rgba": np.full(N * N * 4, 0xA5, np.uint8), "hist": np.full(128, 7, np.uint64),
                     "density": np.full(8 * 8, 7, np.uint32)}
        self.want = {k: v.copy() for k, v in self.host.items()}
        self.dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v)
                    .to("cuda:0") for k, v in self.want.items()}
        torch.cuda.synchronize()

    def ptr(self, name, device):
        return self.dev[name].data_ptr() if device else self.host[name].ctypes.data

    def untouched(self, device):
        if not device:
            return all(np.array_equal(self.host[k], w) for k, w in self.want.items())
        self.torch.cuda.synchronize()
        return all(np.array_equal(self.dev[k].cpu().numpy().view(w.dtype), w) for k, w in self.want.items())


@pytest.fixture(scope="module")
def buffers(gpu):
    return Buffers()


@pytest.fixture(scope="module")
def orbit():
    return DeepOrbit("0", "1", 100, precision_bits=128)


PALETTE = np.arange(4 * 777, dtype=np.uint32).astype(np.uint8)
LUT = np.linspace(0.0, 1.0, 1 << 12)


def _call(gpu, orbit, buffers, kind, op, change):
    f = dict(dict(VIEW[kind], **GEOMETRY), **change)
    lib = gpu._lib
    cv = STRUCT[kind](*[f[k] for k, _ in STRUCT[kind]._fields_])
    device = op.endswith("launch")
    ctx = None if "ctx" in change else gpu._h
    mrd = f.get("mrd", MRD)
    args = [ctx] + ([f.get("slot", 1)] if op == "submit" else []) + \
           ([None if "orbit" in change else orbit._h] if kind in ("deep", "wide") else []) + [None if "view" in change else C.byref(cv)] + \
           (list(f.get("c", (-0.8, 0.156))) if kind == "julia" else [])
    stats = L.mbk_stats()
    tail = [None] if device else [C.byref(stats)]
    keep = []

    def out(name):
        return None if change.get("out", 0) is None else buffers.ptr(name, device) + f.get("misalign", 0)

    if op in ("launch", "compute", "submit"):
        args += [mrd, f.get("flags", BOTH), None if "counts" in change else buffers.ptr("counts", device),
                 None if "bytes" in change else buffers.ptr("bytes", device)] + ([] if op == "submit" else [None] + tail)
    elif op.startswith("hist"):
        args += [mrd, f.get("flags", 0), out("hist")] + tail
    elif op.startswith("density"):
        target = L.mbk_density_target(f.get("t_start_r", -2.0), -2.0, 4.0, f.get("t_range_i", 4.0), f.get("t_width", 8), f.get("t_height", 8))
        keep.append(target)
        args += [None if "target" in change else C.byref(target), mrd, f.get("min_count", 1), f.get("max_count", 0), f.get("flags", 0),
                 out("density")] + (tail if device else tail + [None])
    else:
        eq = op.startswith("eq")
        spec = L.mbk_render_spec(f.get("source", L.MBK_RENDER_EQUALIZED if eq else L.MBK_RENDER_SMOOTH), f.get("supersample", 1),
                                 None if "palette" in change else PALETTE.ctypes.data, f.get("palette_len", 777),
                                 (C.c_uint8 * 4)(1, 2, 3, 255), f.get("scale", 1.0), f.get("offset", 0.0), 0)
        keep.append(spec)
        args += [mrd, f.get("flags", 0), None if "spec" in change else C.byref(spec)]
        if eq:
            lut = LUT[:mrd + 2].copy() if mrd + 2 <= LUT.size else LUT[:2].copy()
            if "lut_entry" in f:
                lut[mrd // 2] = f["lut_entry"]
            keep.append(lut)
            args += [None if "lut" in change else lut.ctypes.data, f.get("lut_len", lut.size)]
        args += [out("rgba")] + tail
    st = getattr(lib, PREFIX[kind] + NAME[op])(*args)
    return st, _error_text(lib, ctx), device


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_refusal(gpu, orbit, buffers, case):
    kind, op, change, message = case
    st, text, device = _call(gpu, orbit, buffers, kind, op, change)
    assert (st, text) == (L.MBK_ERR_INVALID, message)
    assert buffers.untouched(device)


def test_the_table_covers_every_call_and_the_unchanged_calls_are_served(gpu, orbit):
    """Every call of the table, unchanged, is served on 16 x 16 pixels (the refusals are the changes' doing; the ctx still works)."""
    buffers = Buffers()
    seen = {(kind, op) for kind, op, _, _ in CASES}
    assert len(seen) == 3 * 3 + 4 * 6 + 2
    for kind, op in sorted(seen):
        st, text, _ = _call(gpu, orbit, buffers, kind, op, dict(slot=1) if op == "submit" else {})
        assert (st, text if st else "") == (L.MBK_OK, ""), (kind, op)
        if op == "submit":
            gpu.wait(1)
    buffers.torch.cuda.synchronize()
