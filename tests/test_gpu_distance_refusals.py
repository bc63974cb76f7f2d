"""What the distance calls of the C ABI refuse, call by call: the status, the exact text (device._error_text) and outputs left as
they were.  One table of (rule, call, what differs from a served call, message) over the value calls of the six distance rules
(plain, Julia, deep, deep with bilinear approximation, extended-range, extended-range with bilinear approximation) and the
renders of the four that have calls of their own; test_gpu_refusals.py holds the generic renders that serve the other two.
The table records what the calls did before they shared one scaffold, oddities included (the plain rule's own texts and order,
the flags its compute form masks away); the refusals launch nothing."""
import ctypes as C

import numpy as np
import pytest

from distributedmandelbrot_amd import DeepOrbit
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import _error_text

pytestmark = pytest.mark.gpu

MRD, N = 50, 16
BOTH = L.MBK_WANT_COUNTS | L.MBK_WANT_BYTES
F32, LAZY, BLA, XBLA = L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_DEEP_BLA, L.MBK_DEEP_XBLA
ASM, GROUP, SIMPLE, REFILL, SCAN = L.MBK_KERNEL_ASM, L.MBK_KERNEL_GROUP, L.MBK_KERNEL_SIMPLE, L.MBK_KERNEL_REFILL, L.MBK_KERNEL_SCAN
KIND = {"plain": "plain", "julia": "julia", "deep": "deep", "deep_bla": "deep", "wide": "wide", "wide_xbla": "wide"}
VALUE = {"plain": "mbk_view_{}_distance", "julia": "mbk_julia_view_{}_distance", "deep": "mbk_deep_view_{}_distance",
         "deep_bla": "mbk_deep_view_{}_distance_bla", "wide": "mbk_deep_xview_{}_distance", "wide_xbla": "mbk_deep_xview_{}_distance_xbla"}
RENDER = {"julia": "mbk_julia_view_distance_render_{}", "deep_bla": "mbk_deep_view_distance_bla_render_{}",
          "wide": "mbk_deep_xview_distance_render_{}", "wide_xbla": "mbk_deep_xview_distance_xbla_render_{}"}
SOURCE = {"julia": L.MBK_RENDER_DISTANCE, "deep_bla": L.MBK_RENDER_DISTANCE_REL, "wide": L.MBK_RENDER_DISTANCE_REL,
          "wide_xbla": L.MBK_RENDER_DISTANCE_REL}
VIEW = {"plain": dict(start_r=-1.6, start_i=-1.2, range_r=3.2, range_i=2.4), "julia": dict(start_r=-1.6, start_i=-1.2, range_r=3.2, range_i=2.4),
        "deep": dict(range_r=1e-20, range_i=1e-20), "wide": dict(range_r=1.0, range_i=1.0, exp2=-50)}
GEOMETRY = dict(width=N, height=N, col0=0, row0=0, ncols=N, nrows=N)
STRUCT = {"plain": L.mbk_view, "julia": L.mbk_view, "deep": L.mbk_deep_view, "wide": L.mbk_deep_xview}

# ---- the messages -------------------------------------------------------------------------------------------------------
INT32 = "mrd must fit int32 (calc_mb_value returns int32)"
COORD = "view coordinates must be finite and |x| <= 2^500"
TOO_DEEP = "mrd exceeds the mrd the reference orbit was computed for"
SELECTOR = "unknown MBK_KERNEL_* selector"
RANGE = {"deep": "deep view ranges must be finite and lie in [2^-960, 4]",
         "wide": "extended-range deep view ranges must be finite and lie in [2^-64, 4]", "plain": COORD, "julia": COORD}
EXP2 = "extended-range deep view exp2 must lie in [-8192, 0]"
JULIA_PARAMETER = "the Julia parameter must be finite"
PLAIN_XBLA = "MBK_DEEP_XBLA is a flag of the extended-range deep view calls"
PLAIN_F32 = "distance estimates are implemented in binary64 only"
PLAIN_KERNELS = "distance estimates are implemented with the scan / asm / group kernels only"
JULIA_FLAGS = "Julia distance estimates take kernel selection only (binary64; no MBK_LAZY_UNIFORM, no MBK_DEEP_BLA / MBK_DEEP_XBLA)"
JULIA_KERNELS = "Julia views are implemented by MBK_KERNEL_DEFAULT / _ASM / _GROUP only"
DEEP_FLAGS = "deep distance estimates take no flags (no kernel selection, no fp32)"
BLA_NAME = "the _distance_bla calls take no flags: the name selects the rule (MBK_DEEP_BLA is a flag of the count calls)"
WIDE_FLAGS = "extended-range deep distance estimates take no flags (no kernel selection, no fp32)"
WIDE_BLA = "MBK_DEEP_BLA is not implemented for extended-range deep views"
WIDE_XBLA = "MBK_DEEP_XBLA is not implemented for extended-range deep distance estimates"
XBLA_NAME = "the _distance_xbla calls take no flags: the name selects the rule (MBK_DEEP_XBLA is a flag of the count calls)"
# every flag a rule refuses, with the text it draws: on the value calls and, through the sample view, on the rule's renders
FLAGS = {
    # (the plain rule lets MBK_DEEP_BLA, MBK_LAZY_UNIFORM and MBK_WANT_* through; its compute form MBK_PRECISION_F32 too: see
    # test_the_flags_the_plain_rule_lets_through_are_served)
    "plain": [(XBLA, PLAIN_XBLA), (XBLA | F32, PLAIN_XBLA), (SIMPLE, PLAIN_KERNELS), (REFILL, PLAIN_KERNELS), (0x600, SELECTOR),
              (0x700, SELECTOR)],
    "julia": [(BLA, JULIA_FLAGS), (XBLA, JULIA_FLAGS), (F32, JULIA_FLAGS), (LAZY, JULIA_FLAGS), (L.MBK_WANT_COUNTS, JULIA_FLAGS),
              (L.MBK_WANT_BYTES, JULIA_FLAGS), (SCAN | F32, JULIA_FLAGS), (SCAN, JULIA_KERNELS), (SIMPLE, JULIA_KERNELS),
              (REFILL, JULIA_KERNELS), (0x600, JULIA_KERNELS)],
    "deep": [(BLA, DEEP_FLAGS), (XBLA, DEEP_FLAGS), (F32, DEEP_FLAGS), (LAZY, DEEP_FLAGS), (GROUP, DEEP_FLAGS), (ASM, DEEP_FLAGS),
             (L.MBK_WANT_COUNTS, DEEP_FLAGS), (L.MBK_WANT_BYTES, DEEP_FLAGS)],
    "deep_bla": [(BLA, BLA_NAME), (BLA | GROUP, BLA_NAME), (XBLA, DEEP_FLAGS), (F32, DEEP_FLAGS), (LAZY, DEEP_FLAGS), (GROUP, DEEP_FLAGS),
                 (ASM, DEEP_FLAGS), (L.MBK_WANT_COUNTS, DEEP_FLAGS), (L.MBK_WANT_BYTES, DEEP_FLAGS)],
    "wide": [(XBLA, WIDE_XBLA), (XBLA | BLA, WIDE_XBLA), (BLA, WIDE_BLA), (BLA | GROUP, WIDE_BLA), (F32, WIDE_FLAGS), (LAZY, WIDE_FLAGS),
             (GROUP, WIDE_FLAGS), (ASM, WIDE_FLAGS), (L.MBK_WANT_COUNTS, WIDE_FLAGS), (L.MBK_WANT_BYTES, WIDE_FLAGS)],
    "wide_xbla": [(XBLA, XBLA_NAME), (XBLA | BLA, XBLA_NAME), (BLA, WIDE_BLA), (BLA | GROUP, WIDE_BLA), (F32, WIDE_FLAGS),
                  (LAZY, WIDE_FLAGS), (GROUP, WIDE_FLAGS), (ASM, WIDE_FLAGS), (L.MBK_WANT_COUNTS, WIDE_FLAGS), (L.MBK_WANT_BYTES, WIDE_FLAGS)],
}
# one refused flag per rule, for the cases with two faults, and its text
BAD_FLAG = {"plain": (SIMPLE, PLAIN_KERNELS), "julia": (F32, JULIA_FLAGS), "deep": (GROUP, DEEP_FLAGS), "deep_bla": (GROUP, DEEP_FLAGS),
            "wide": (GROUP, WIDE_FLAGS), "wide_xbla": (GROUP, WIDE_FLAGS)}
ONLY = {"julia": "Julia distance renders take MBK_RENDER_DISTANCE only",
        "deep_bla": "deep distance renders with bilinear approximation take MBK_RENDER_DISTANCE_REL only",
        "wide": "extended-range deep distance renders take MBK_RENDER_DISTANCE_REL only",
        "wide_xbla": "extended-range deep distance renders with bilinear approximation take MBK_RENDER_DISTANCE_REL only"}
NAN, INF = float("nan"), float("inf")


def _cases():
    out = []

    def add(rule, ops, message, **change):
        out.extend((rule, op, change, message) for op in ops)

    for rule, kind in KIND.items():
        values = ("launch", "compute")
        renders = ("render_launch", "render_compute") if rule in RENDER else ()
        every = values + renders
        plain, deep = rule == "plain", kind in ("deep", "wide")
        flag, flag_text = BAD_FLAG[rule]
        # the pointers of the value calls: the plain pair has one text for all of them, and its compute form counts the view in
        add(rule, values, "NULL argument" if plain else "ctx is NULL", ctx=None)
        add(rule, values, "NULL argument" if plain else "NULL value pointer", out=None)
        add(rule, values, "NULL argument" if plain else "ctx is NULL", ctx=None, out=None)
        add(rule, values, "NULL argument" if plain else "NULL value pointer", out=None, view=None)
        add(rule, values, "NULL argument" if plain else "NULL value pointer", out=None, flags=flag)
        if plain:
            add(rule, ("launch",), "view is NULL", view=None)
            add(rule, ("compute",), "NULL argument", view=None)
        else:
            add(rule, every, "view is NULL", view=None)
        if deep:
            add(rule, every, "orbit is NULL", orbit=None)
            add(rule, values, "orbit is NULL", orbit=None, view=None)
            add(rule, renders, "view is NULL", orbit=None, view=None)       # a render looks at the output window first
            add(rule, values, "orbit is NULL", orbit=None, range_r=NAN)
            add(rule, every, flag_text, orbit=None, flags=flag)             # the flags come before the pointers of the view
        # the view and its window
        add(rule, every, "empty view", width=0, height=0, ncols=0, nrows=0)
        add(rule, values, "empty view", width=0)
        add(rule, renders, "window exceeds the view", width=0)
        add(rule, every, "empty window", ncols=0)
        add(rule, every, "empty window", nrows=0)
        add(rule, every, "window exceeds the view", col0=10, ncols=7)
        add(rule, every, "window exceeds the view", row0=N, nrows=1)
        add(rule, every, RANGE[kind], range_r=NAN)
        add(rule, every, RANGE[kind], range_i=INF)
        if deep:
            add(rule, every, RANGE[kind], range_r=2.0 ** (-961 if kind == "deep" else -65))
            add(rule, every, RANGE[kind], range_i=4.5)
            add(rule, every, TOO_DEEP, mrd=101)
            add(rule, every, "empty view", width=0, height=0, ncols=0, nrows=0, mrd=101)
            add(rule, every, RANGE[kind], range_r=NAN, mrd=101)
        else:
            add(rule, every, INT32, mrd=1 << 31)
            add(rule, every, COORD, range_r=NAN, mrd=1 << 31)
        if kind == "wide":
            add(rule, every, EXP2, exp2=1)
            add(rule, every, EXP2, exp2=-8193)
            add(rule, every, RANGE[kind], exp2=1, range_r=NAN)
        if kind == "julia":
            add(rule, every, JULIA_PARAMETER, c=(NAN, 0.0))
            add(rule, every, JULIA_PARAMETER, c=(0.0, INF))
            add(rule, values, JULIA_PARAMETER, c=(NAN, 0.0), view=None)     # the parameter comes before the view
            add(rule, every, JULIA_PARAMETER, c=(NAN, 0.0), ncols=0)
            add(rule, every, flag_text, flags=flag, c=(NAN, 0.0))
            add(rule, every, JULIA_KERNELS, flags=SCAN, c=(NAN, 0.0))
            add(rule, every, JULIA_KERNELS, flags=SCAN, mrd=1 << 31)         # mrd too large, bad selector: the selector first
        # the flags
        for flags, message in FLAGS[rule]:
            add(rule, every, message, flags=flags)
        if plain:
            add(rule, ("launch",), PLAIN_F32, flags=F32)                    # (the compute form masks the flag away and serves the call)
            add(rule, ("launch",), PLAIN_F32, flags=F32 | SIMPLE)
            add(rule, ("compute",), PLAIN_KERNELS, flags=F32 | SIMPLE)
            add(rule, every, INT32, flags=0x600, mrd=1 << 31)               # mrd too large, bad selector: mrd first
            add(rule, every, "empty window", flags=flag, ncols=0)           # the plain rule looks at the view first
            add(rule, every, COORD, flags=flag, range_r=NAN)
            add(rule, ("launch",), "view is NULL", flags=flag, view=None)
        else:
            add(rule, every, flag_text, flags=flag, ncols=0)                # every other rule looks at its flags first
            add(rule, every, flag_text, flags=flag, range_r=NAN)
            add(rule, values, flag_text, flags=flag, view=None)
            add(rule, every, flag_text, flags=flag, mrd=101 if deep else 1 << 31)
        # the renders
        add(rule, renders, "ctx is NULL", ctx=None)
        add(rule, renders, "ctx is NULL", ctx=None, spec=None)
        add(rule, renders, "render spec is NULL", spec=None)
        add(rule, renders, "render spec is NULL", spec=None, view=None)
        add(rule, renders, "palette is NULL", palette=None)
        add(rule, renders, "palette is NULL", palette=None, source=L.MBK_RENDER_SMOOTH)
        add(rule, renders, "supersample must be 1, 2, 3, 4 or 8", supersample=5)
        add(rule, renders, "supersample must be 1, 2, 3, 4 or 8", supersample=0, ncols=0)
        add(rule, renders, "MBK_RENDER_DISTANCE / _DISTANCE_REL take a palette of 2 .. 65536 entries", palette_len=1)
        add(rule, renders, "scale must lie in (0, 2^80]", scale=INF)
        add(rule, renders, "offset must lie in [-2^20, 2^20]", offset=NAN)
        if renders:
            other = L.MBK_RENDER_DISTANCE_REL if SOURCE[rule] == L.MBK_RENDER_DISTANCE else L.MBK_RENDER_DISTANCE
            add(rule, renders, ONLY[rule], source=other)
            add(rule, renders, ONLY[rule], source=L.MBK_RENDER_SMOOTH)
            add(rule, renders, ONLY[rule], source=L.MBK_RENDER_BYTES, palette_len=256)
            # (the sources the spec's own rules refuse before the rule sees them)
            add(rule, renders, "MBK_RENDER_BYTES takes a palette of 256 entries", source=L.MBK_RENDER_BYTES)
            add(rule, renders, "MBK_RENDER_EQUALIZED needs a table: use the equalized calls", source=L.MBK_RENDER_EQUALIZED)
            add(rule, renders, "unknown MBK_RENDER_* source", source=2)
            add(rule, renders, ONLY[rule], source=other, out=None)           # wrong source, output NULL
            add(rule, renders, ONLY[rule], source=other, flags=flag)
            add(rule, renders, ONLY[rule], source=other, view=None)
        add(rule, renders, "output pointer is NULL", out=None)
        add(rule, renders, "output pointer is NULL", out=None, view=None)
        add(rule, renders, "output pointer is NULL", out=None, width=1 << 31, supersample=2)
        add(rule, renders, "output pointer is NULL", out=None, flags=flag)
        add(rule, renders, "width or height times supersample does not fit 32 bits", width=1 << 31, supersample=2)
        add(rule, renders, "width or height times supersample does not fit 32 bits", height=1 << 30, supersample=4)
        add(rule, renders, "width or height times supersample does not fit 32 bits", width=1 << 31, supersample=2, col0=10, ncols=7, flags=flag)
        add(rule, renders, "window exceeds the view", col0=10, ncols=7, flags=flag)      # window exceeds, bad flag
        add(rule, renders, "window exceeds the view", row0=N, nrows=1, mrd=101 if deep else 1 << 31)
        add(rule, renders[:1], "d_rgba must be 4-byte aligned", misalign=2)
        add(rule, renders[:1], flag_text, misalign=2, flags=flag)           # the alignment comes last
        add(rule, renders[:1], "empty window", misalign=2, ncols=0)
    return out


CASES = _cases()


def _id(case):
    rule, op, change, _ = case
    return f"{rule}-{op}-" + ",".join(f"{k}={v:#x}" if k == "flags" else k for k, v in change.items())


class Buffers:
    """Host and device outputs, filled once: a refused call leaves every one of them as it is."""

    def __init__(self):
        import torch
        self.torch = torch
        self.host = {"counts": np.full(N * N, -7, np.int32), "values": np.full(N * N, -7.0), "rgba": np.full(N * N * 4, 0xA5, np.uint8)}
        self.want = {k: v.copy() for k, v in self.host.items()}
        self.dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in self.want.items()}
        torch.cuda.synchronize()

    def ptr(self, name, device):
        return self.dev[name].data_ptr() if device else self.host[name].ctypes.data

    def read(self, name, device):
        self.torch.cuda.synchronize()
        return self.dev[name].cpu().numpy() if device else self.host[name].copy()

    def untouched(self, device):
        return all(np.array_equal(self.read(k, device), w) for k, w in self.want.items())


@pytest.fixture(scope="module")
def buffers(gpu):
    return Buffers()


@pytest.fixture(scope="module")
def orbit():
    return DeepOrbit("0", "1", 100, precision_bits=128)


PALETTE = np.arange(4 * 777, dtype=np.uint32).astype(np.uint8)


def _call(gpu, orbit, buffers, rule, op, change):
    kind = KIND[rule]
    f = dict(dict(VIEW[kind], **GEOMETRY), **change)
    lib = gpu._lib
    cv = STRUCT[kind](*[f[k] for k, _ in STRUCT[kind]._fields_])
    device = op.endswith("launch")
    ctx = None if "ctx" in change else gpu._h
    args = [ctx] + ([None if "orbit" in change else orbit._h] if kind in ("deep", "wide") else []) + \
           [None if "view" in change else C.byref(cv)] + (list(f.get("c", (-0.8, 0.156))) if kind == "julia" else []) + \
           [f.get("mrd", MRD), f.get("flags", 0)]
    stats = L.mbk_stats()
    tail = [None] if device else [C.byref(stats)]

    def out(name):
        return None if change.get("out", 0) is None else buffers.ptr(name, device) + f.get("misalign", 0)

    if op.startswith("render"):
        spec = L.mbk_render_spec(f.get("source", SOURCE[rule]), f.get("supersample", 1), None if "palette" in change else PALETTE.ctypes.data,
                                 f.get("palette_len", 777), (C.c_uint8 * 4)(1, 2, 3, 255), f.get("scale", 1.0), f.get("offset", 0.0), 0)
        args += [None if "spec" in change else C.byref(spec), out("rgba")] + tail
        name = RENDER[rule].format(op[len("render_"):])
    else:
        args += [buffers.ptr("counts", device), out("values")] + tail
        name = VALUE[rule].format(op)
    st = getattr(lib, name)(*args)
    return st, _error_text(lib, ctx), device


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_refusal(gpu, orbit, buffers, case):
    rule, op, change, message = case
    st, text, device = _call(gpu, orbit, buffers, rule, op, change)
    assert (st, text) == (L.MBK_ERR_INVALID, message)
    assert buffers.untouched(device)


def test_the_flags_the_plain_rule_lets_through_are_served(gpu, orbit):
    """The plain rule refuses none of MBK_DEEP_BLA, MBK_LAZY_UNIFORM and MBK_WANT_*, and mbk_view_compute_distance masks its flags
    to the kernel selector and MBK_DEEP_XBLA before it checks them, so MBK_PRECISION_F32 -- which mbk_view_launch_distance
    refuses -- is served there: each such call gives what the call without the flag gives."""
    for op, flags in (("compute", (F32, BLA, LAZY, BOTH, F32 | GROUP)), ("launch", (BLA, LAZY, BOTH, BLA | GROUP))):
        want = None
        for f in (0,) + flags:
            buffers = Buffers()
            st, text, device = _call(gpu, orbit, buffers, "plain", op, dict(flags=f))
            assert (st, text if st else "") == (L.MBK_OK, ""), (op, hex(f))
            got = [buffers.read(k, device) for k in ("counts", "values")]
            want = want or got
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (op, hex(f))
            assert not np.array_equal(got[0], buffers.want["counts"]) and buffers.read("rgba", device).tolist() == buffers.want["rgba"].tolist()


def test_the_table_covers_every_call_and_the_unchanged_calls_are_served(gpu, orbit):
    """Every call of the table, unchanged, is served on 16 x 16 pixels (the refusals are the changes' doing; the ctx still works)."""
    buffers = Buffers()
    seen = {(rule, op) for rule, op, _, _ in CASES}
    assert len(seen) == 6 * 2 + 4 * 2
    for rule, op in sorted(seen):
        st, text, _ = _call(gpu, orbit, buffers, rule, op, {})
        assert (st, text if st else "") == (L.MBK_OK, ""), (rule, op)
    buffers.torch.cuda.synchronize()
    assert not buffers.untouched(True) and not buffers.untouched(False)
