"""The catalogue of launch forms that the GPU tests of captures (test_gpu_graph.py) and of streams (test_gpu_streams.py) share.

A Case is one *_launch form on fixed arguments: outs() makes its device outputs with guard elements around them, launch(dev, outs,
stream) enqueues it on a hipStream_t, want(dev) gives what the synchronous form stores for the same arguments.  The builders below
make the cases of every family at the smallest shapes at which each path exists; _check compares byte for byte, guards included.

A plain module like the *_model.py files: no test, no fixture.  torch is imported where a device output is made, so the module
imports -- and the GPU files collect -- without a GPU.
"""
from dataclasses import dataclass
from typing import Callable

import numpy as np

from distributedmandelbrot_amd import DeepOrbit, DeepView, DensityTarget, Palette, View, WideDeepView
from distributedmandelbrot_amd.image import equalize_lut

GUARD = 64
SENTINEL = {"i4": -5, "u1": 0xA5, "f8": -77.0, "i8": 0x5A5A5A5A5A5A5A5A, "rgba": 0x5A5A5A5A}


class Out:
    """One device output of n elements with GUARD sentinel elements in front of and behind it."""

    def __init__(self, kind: str, n: int):
        import torch
        dtype = {"i4": torch.int32, "u1": torch.uint8, "f8": torch.float64, "i8": torch.int64, "rgba": torch.int32}[kind]
        self.n, self.sentinel = int(n), SENTINEL[kind]
        self.t = torch.full((self.n + 2 * GUARD,), self.sentinel, dtype=dtype, device="cuda:0")

    @property
    def ptr(self) -> int:
        return self.t[GUARD:].data_ptr()

    def refill(self) -> None:
        self.t.fill_(self.sentinel)

    def zero_body(self) -> None:
        self.t[GUARD:GUARD + self.n].zero_()

    def body(self) -> np.ndarray:
        return self.t.cpu().numpy()[GUARD:GUARD + self.n]

    def guards_intact(self) -> bool:
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == self.sentinel).all() and (h[GUARD + self.n:] == self.sentinel).all())

    def untouched(self) -> bool:
        return bool((self.t.cpu().numpy() == self.sentinel).all())


@dataclass
class Case:
    """A launch form on fixed arguments: outs() makes its device outputs, launch(dev, outs, stream) enqueues it on the hipStream_t
    `stream`, want(dev) gives what the synchronous form stores for the same arguments, by output name."""
    outs: Callable
    launch: Callable
    want: Callable
    times: int = 1      # as an interposed launch: how often it is enqueued


def _bytes(a) -> bytes:
    return np.ascontiguousarray(a).tobytes()


def _check(outs, want, what, factor: int = 1):
    for name, o in outs.items():
        assert o.guards_intact(), (what, name, "guard elements written")
        if name not in want:
            assert o.untouched(), (what, name)
            continue
        w = np.ascontiguousarray(want[name])
        got = o.body()
        if factor != 1:
            w = (w.astype(np.uint64) * np.uint64(factor)).astype(w.dtype)
        same = _bytes(got) == _bytes(w)
        assert same, (what, name, int((np.frombuffer(_bytes(got), np.uint8) != np.frombuffer(_bytes(w), np.uint8)).sum()), "bytes differ")
    assert set(want) <= set(outs), (what, set(want) - set(outs))


# ---- plain views --------------------------------------------------------------------------------------------------------------

SEAHORSE = ((-0.765, 0.085, 0.04, 0.04 * 44 / 66, 67, 45), 600)      # neither side a multiple of 8 (tests/test_gpu_relief.py)
FULL = (-2.0, -1.5, 3.0, 3.0)


def _px(v, window):
    return (window[2] * window[3]) if window is not None else v[4] * v[5]


def plain(v, mrd, kernel, outputs, window=None, times=1, precision="f64") -> Case:
    """mbk_view_launch ("counts", "bytes", "counts+bytes") or mbk_view_launch_smooth ("smooth": nu and counts)."""
    view, n = View(*v), _px(v, window)
    if outputs == "smooth":
        def want(dev):
            nu, counts, _ = dev.compute_view_smooth(view, mrd, window=window, kernel=kernel)
            return {"smooth": nu, "counts": counts}
        return Case(lambda: {"smooth": Out("f8", n), "counts": Out("i4", n)},
                    lambda dev, o, s: dev.launch_view_smooth(view, mrd, d_smooth=o["smooth"].ptr, d_counts=o["counts"].ptr, stream=s,
                                                             window=window, kernel=kernel), want, times)
    wc, wb = "counts" in outputs, "bytes" in outputs

    def want(dev):
        counts, byts, _ = dev.compute_view(view, mrd, window=window, want_counts=wc, want_bytes=wb, kernel=kernel, precision=precision)
        return dict(([("counts", counts)] if wc else []) + ([("bytes", byts)] if wb else []))
    return Case(lambda: dict(([("counts", Out("i4", n))] if wc else []) + ([("bytes", Out("u1", n))] if wb else [])),
                lambda dev, o, s: dev.launch_view(view, mrd, d_counts=o["counts"].ptr if wc else 0, d_bytes=o["bytes"].ptr if wb else 0,
                                                  stream=s, window=window, kernel=kernel, precision=precision), want, times)


def _ordered_mrd(dev):
    return 2 * dev.get_option("probe_steps") + 2


# ---- two-pass plain calls and Julia views ------------------------------------------------------------------------------------------

RAGGED = (5, 3, 21, 17)
BLOCKS = ((-0.4, 0.2, 0.6, 0.6, 64, 64), 300)      # whole-interior 8 x 8 blocks and the edge (tests/test_gpu_relief.py)
INTERIOR = ((-2.0, -1.5, 3.0, 3.0, 61, 45), 600)   # tests/test_gpu_interior.py
JULIA = ((-1.7, -1.3, 3.4, 2.6, 64, 48), (-0.8, 0.156), 300)


def distance(v, mrd, kernel, window=None, with_counts=True) -> Case:
    view, n = View(*v), _px(v, window)

    def want(dev):
        de, counts, _ = dev.compute_view_distance(view, mrd, window=window, kernel=kernel)
        return {"distance": de, "counts": counts} if with_counts else {"distance": de}
    return Case(lambda: {"distance": Out("f8", n), "counts": Out("i4", n)},
                lambda dev, o, s: dev.launch_view_distance(view, mrd, d_distance=o["distance"].ptr, d_counts=o["counts"].ptr if with_counts else 0,
                                                           stream=s, window=window, kernel=kernel), want)


def normals(v, mrd, kernel, window=None) -> Case:
    """NULL d_counts: the counts of the two-pass form live in the stream's scratch."""
    view, n = View(*v), _px(v, window)

    def want(dev):
        _, nrm, de, _ = dev.compute_view_normals(view, mrd, window=window, kernel=kernel, want_distance=True)
        return {"normals": nrm, "distance": de}
    return Case(lambda: {"normals": Out("f8", 2 * n), "distance": Out("f8", n)},
                lambda dev, o, s: dev.launch_view_normals(view, mrd, d_normals=o["normals"].ptr, d_distance=o["distance"].ptr, stream=s,
                                                          window=window, kernel=kernel), want)


def interior(v, mrd, kernel, window=None) -> Case:
    view, n = View(*v), _px(v, window)

    def want(dev):
        period, de, _, _ = dev.compute_view_interior(view, mrd, window=window, kernel=kernel)
        return {"period": period, "distance": de}
    return Case(lambda: {"period": Out("i4", n), "distance": Out("f8", n)},
                lambda dev, o, s: dev.launch_view_interior(view, mrd, d_period=o["period"].ptr, d_distance=o["distance"].ptr, stream=s,
                                                           window=window, kernel=kernel), want)


def julia(v, c, mrd, kernel, window=None) -> Case:
    view, n = View(*v), _px(v, window)

    def want(dev):
        counts, byts, nu, _ = dev.compute_julia_view(view, c, mrd, window=window, want_smooth=True, kernel=kernel)
        return {"counts": counts, "bytes": byts, "smooth": nu}
    return Case(lambda: {"counts": Out("i4", n), "bytes": Out("u1", n), "smooth": Out("f8", n)},
                lambda dev, o, s: dev.launch_julia_view(view, c, mrd, d_counts=o["counts"].ptr, d_bytes=o["bytes"].ptr,
                                                        d_smooth=o["smooth"].ptr, stream=s, window=window, kernel=kernel), want)


def julia_distance(v, c, mrd, kernel, window=None) -> Case:
    view, n = View(*v), _px(v, window)

    def want(dev):
        return {"distance": dev.compute_julia_view_distance(view, c, mrd, window=window, kernel=kernel)[0]}
    return Case(lambda: {"distance": Out("f8", n)},
                lambda dev, o, s: dev.launch_julia_view_distance(view, c, mrd, d_distance=o["distance"].ptr, stream=s, window=window,
                                                                 kernel=kernel), want)


# ---- deep and extended-range deep views ------------------------------------------------------------------------------------------

_ORBITS = {}


def _deep(w=64, h=64):
    """(orbit, view, a view of the same orbit with another dcmax, mrd): the seahorse case of tests/test_gpu_deep_relief.py."""
    if "deep" not in _ORBITS:
        _ORBITS["deep"] = DeepOrbit("-0.77568377", "0.13646737", 3000, min_span=1e-12)
    return _ORBITS["deep"], DeepView(1e-12, w, h), DeepView(2e-12, w, h), 3000


def _wide(w=64, h=64):
    """The same for an extended-range view: the case "i-1100" of tests/test_gpu_deep_wide_relief.py."""
    if "wide" not in _ORBITS:
        _ORBITS["wide"] = DeepOrbit("0", "1", 3000, min_span_exp2=WideDeepView(1.0, -1100, 64, 64).min_span_exp2)
    return _ORBITS["wide"], WideDeepView(1.0, -1100, w, h), WideDeepView(1.0, -1099, w, h), 3000


def deep(orbit, view, mrd, kind, table, window=None) -> Case:
    """The launch forms of a deep or an extended-range deep view; table: MBK_DEEP_BLA / MBK_DEEP_XBLA."""
    wide = isinstance(view, WideDeepView)
    n = (window[2] * window[3]) if window is not None else view.width * view.height
    flag = {"xbla": table} if wide else {"bla": table}
    if kind == "counts":
        def want(dev):
            counts, _, nu, _ = dev.compute_deep_view(orbit, view, mrd, window=window, want_bytes=False, want_smooth=True, **flag)
            return {"counts": counts, "smooth": nu}
        return Case(lambda: {"counts": Out("i4", n), "smooth": Out("f8", n)},
                    lambda dev, o, s: dev.launch_deep_view(orbit, view, mrd, d_counts=o["counts"].ptr, d_smooth=o["smooth"].ptr, stream=s,
                                                           window=window, **flag), want)
    if kind == "distance":
        name = ("wide_view_distance" + ("_xbla" if table else "")) if wide else ("deep_view_distance" + ("_bla" if table else ""))

        def want(dev):
            rel, counts, _ = getattr(dev, "compute_" + name)(orbit, view, mrd, window=window)
            return {"rel": rel, "counts": counts}
        return Case(lambda: {"rel": Out("f8", n), "counts": Out("i4", n)},
                    lambda dev, o, s: getattr(dev, "launch_" + name)(orbit, view, mrd, d_rel=o["rel"].ptr, d_counts=o["counts"].ptr, stream=s,
                                                                     window=window), want)
    if kind == "normals":
        name = "wide_view_normals" if wide else "deep_view_normals"

        def want(dev):
            counts, nrm, nu, rel, _ = getattr(dev, "compute_" + name)(orbit, view, mrd, window=window, want_smooth=True, want_distance=True, **flag)
            return {"counts": counts, "normals": nrm, "smooth": nu, "rel": rel}
        return Case(lambda: {"counts": Out("i4", n), "normals": Out("f8", 2 * n), "smooth": Out("f8", n), "rel": Out("f8", n)},
                    lambda dev, o, s: getattr(dev, "launch_" + name)(orbit, view, mrd, d_normals=o["normals"].ptr, d_counts=o["counts"].ptr,
                                                                     d_smooth=o["smooth"].ptr, d_rel=o["rel"].ptr, stream=s, window=window,
                                                                     **flag), want)
    assert kind == "nucleus" and not table
    name = "wide_view_nucleus" if wide else "deep_view_nucleus"

    def want(dev):
        period, delta, counts, _ = getattr(dev, "compute_" + name)(orbit, view, mrd, window=window)
        return {"period": period, "delta": delta, "counts": counts}
    return Case(lambda: {"period": Out("i4", n), "delta": Out("f8", 2 * n), "counts": Out("i4", n)},
                lambda dev, o, s: getattr(dev, "launch_" + name)(orbit, view, mrd, d_period=o["period"].ptr, d_delta=o["delta"].ptr,
                                                                 d_counts=o["counts"].ptr, stream=s, window=window), want)


DEEP_KINDS = [("counts", False), ("counts", True), ("distance", False), ("distance", True), ("normals", False), ("normals", True),
              ("nucleus", False)]


# ---- renders -------------------------------------------------------------------------------------------------------------------

RENDER_VIEW = ((-0.765, 0.085, 0.04, 0.04 * 27 / 39, 40, 28), 400)       # tests/test_gpu_relief.py
BANDS = 10                                                                 # 28 rows: three bands


def _render_palette():
    rng = np.random.RandomState(11)
    return Palette(rng.randint(0, 256, (53, 4)).astype(np.uint8), inside=(9, 8, 7, 200), scale=3.7, offset=0.25)


def _image(n, mask=False):
    return (lambda: {"rgba": Out("rgba", n), "mask": Out("u1", n)}) if mask else (lambda: {"rgba": Out("rgba", n)})


def _rgba(img):
    return {"rgba": np.ascontiguousarray(img).view(np.int32).ravel()}


def render(kind_of_view, what, pal, *, s=2, rows=0, window=None, threshold=0, kernel="default", lut=None) -> Case:
    """A render launch of a plain view ("plain"), the Julia set ("julia"), a deep view with MBK_DEEP_BLA ("deep") or an
    extended-range view with MBK_DEEP_XBLA ("wide").  what: "smooth", "distance", "equalized" (with `lut`), "relief", "interior",
    "adaptive".  The expected image is the synchronous form's."""
    if kind_of_view in ("plain", "julia"):
        view, mrd = View(*RENDER_VIEW[0]), RENDER_VIEW[1]
        if kind_of_view == "julia":
            view, c, mrd = View(*JULIA[0][:4], 40, 28), JULIA[1], JULIA[2]
        orbit = None
    else:
        orbit, view, _, mrd = _deep(40, 28) if kind_of_view == "deep" else _wide(40, 28)
    n = (window[2] * window[3]) if window is not None else view.width * view.height
    common = dict(palette=pal, supersample=s, window=window, max_band_rows=rows)
    table = {"deep": {"bla": True}, "wide": {"xbla": True}}.get(kind_of_view, {})
    lead = (orbit, view, mrd) if orbit is not None else ((view, c, mrd) if kind_of_view == "julia" else (view, mrd))
    if kind_of_view in ("plain", "julia"):
        common["kernel"] = kernel
    if what == "adaptive":
        name = {"plain": "render_view_adaptive", "deep": "render_deep_view_adaptive", "wide": "render_wide_view_adaptive"}[kind_of_view]

        def want(dev):
            img, mask, _ = getattr(dev, name)(*lead, threshold=threshold, want_mask=True, **common, **table)
            return dict(_rgba(img), mask=mask)
        return Case(_image(n, mask=True),
                    lambda dev, o, st: getattr(dev, "launch_" + name)(*lead, threshold=threshold, d_rgba=o["rgba"].ptr, d_mask=o["mask"].ptr,
                                                                      stream=st, **common, **table), want)
    if what == "relief":
        name = {"plain": "render_view_relief", "deep": "render_deep_view_relief", "wide": "render_wide_view_relief"}[kind_of_view]
        extra = dict(light_deg=200.0, height=0.75)
    elif what == "interior":
        name, extra = "render_view_interior", dict(scale=64.0)
    elif what == "distance" and kind_of_view != "plain":
        name = {"julia": "render_julia_view_distance", "deep": "render_deep_view_distance_bla", "wide": "render_wide_view_distance_xbla"}[kind_of_view]
        extra, table = {}, {}
    else:
        name = {"plain": "render_view", "julia": "render_julia_view", "deep": "render_deep_view", "wide": "render_deep_view"}[kind_of_view]
        extra = dict(source=what, **({"lut": lut} if what == "equalized" else {}))
    return Case(_image(n), lambda dev, o, st: getattr(dev, "launch_" + name)(*lead, d_rgba=o["rgba"].ptr, stream=st, **common, **extra, **table),
                lambda dev: _rgba(getattr(dev, name)(*lead, **common, **extra, **table)[0]))


def _lut(dev, kind_of_view):
    """The equalisation table of the whole view at output resolution: what the synchronous form takes when none is given."""
    if kind_of_view == "plain":
        return equalize_lut(dev.view_histogram(View(*RENDER_VIEW[0]), RENDER_VIEW[1]))
    if kind_of_view == "julia":
        return equalize_lut(dev.julia_view_histogram(View(*JULIA[0][:4], 40, 28), JULIA[1], JULIA[2]))
    orbit, view, _, mrd = _deep(40, 28) if kind_of_view == "deep" else _wide(40, 28)
    return equalize_lut(dev.deep_view_histogram(orbit, view, mrd, bla=kind_of_view == "deep", xbla=kind_of_view == "wide"))


RENDERS = ([(k, w, 2, 0, 0) for k in ("plain", "deep", "wide") for w in ("smooth", "distance", "equalized", "relief")]
           + [(k, "adaptive", s, t, 0) for k in ("plain", "deep", "wide") for s in (2, 3) for t in (16, 0)]
           + [("julia", w, 2, 0, 0) for w in ("smooth", "distance", "equalized")]
           + [("plain", "interior", 2, 0, 0)]
           + [(k, w, 2, 16, BANDS) for k in ("plain", "deep", "wide") for w in ("smooth", "relief", "adaptive")])


# ---- accumulating calls ----------------------------------------------------------------------------------------------------------

def histogram(kind_of_view, window=None) -> Case:
    if kind_of_view == "plain":
        lead, mrd, kw, name = (View(*SEAHORSE[0]), SEAHORSE[1]), SEAHORSE[1], {}, "view_histogram"
    elif kind_of_view == "julia":
        lead, mrd, kw, name = (View(*JULIA[0]), JULIA[1], JULIA[2]), JULIA[2], {}, "julia_view_histogram"
    else:
        orbit, view, _, mrd = _deep() if kind_of_view == "deep" else _wide()
        lead, kw, name = (orbit, view, mrd), ({"bla": True} if kind_of_view == "deep" else {"xbla": True}), "deep_view_histogram"
    return Case(lambda: {"hist": Out("i8", mrd)},
                lambda dev, o, s: getattr(dev, "launch_" + name)(*lead, d_hist=o["hist"].ptr, stream=s, window=window, **kw),
                lambda dev: {"hist": getattr(dev, name)(*lead, window=window, **kw).view(np.int64)})


DENSITY = (View(-2.0, -1.25, 3.0, 2.5, 40, 24), DensityTarget(-2.5, -2.5, 5.0, 5.0, 64, 48), 200)


def density(window) -> Case:
    """mbk_view_density_launch of DENSITY: it ADDS into its table."""
    view, target, mrd = DENSITY
    return Case(lambda: {"table": Out("i4", 64 * 48)},
                lambda dev, o, s: dev.launch_view_density(view, target, mrd, d_density=o["table"].ptr, stream=s, window=window),
                lambda dev: {"table": dev.compute_view_density(view, target, mrd, window=window)[0].view(np.int32).ravel()})


def density_render(d_table, table, pal, mode="sqrt", factor=1) -> Case:
    """mbk_density_render_launch of the device table d_table (a torch tensor), whose host copy is `table` (height x width)."""
    h, w = table.shape
    n = (w // factor) * (h // factor)
    return Case(_image(n), lambda dev, o, s: dev.launch_render_density(d_table.data_ptr(), w, h, palette=pal, d_rgba=o["rgba"].ptr,
                                                                       mode=mode, factor=factor, stream=s),
                lambda dev: _rgba(dev.render_density(table, palette=pal, mode=mode, factor=factor)[0]))


def counts_histogram(d_counts, counts, n, mrd) -> Case:
    """mbk_counts_histogram of the first n of the device counts d_counts (a torch tensor; host copy `counts`): device pointers
    alone, no scratch.  It ADDS into its table."""
    return Case(lambda: {"hist": Out("i8", mrd)},
                lambda dev, o, s: dev.counts_histogram(d_counts.data_ptr(), n, mrd, o["hist"].ptr, stream=s),
                lambda dev: {"hist": np.bincount(counts[:n], minlength=mrd).astype(np.int64)})

