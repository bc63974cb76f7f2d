"""MandelbrotDevice -- one GPU context over the C ABI (include/mbk.h).

Mirrors, for a generic view, what the reference's ``process_workload`` does for a DataChunk tile
(DistributedMandelbrotWorkerCUDA.py:70-100, "WorkerCUDA.py"): coordinates (gen_arrays, :19-37),
the escape-time kernel (calc_mb_value, :39-68) and the uint8 quantiser (:96-98) -- all on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, replace
from decimal import Decimal
from fractions import Fraction
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np

from . import _lib as L


class MbkError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libmbk_hip status {status}: {message}")
        self.status = status


def _error_text(lib, ctx=None) -> str:
    """The library's last error text: that of `ctx`, or (None) of the calling thread."""
    return (lib.mbk_last_error(ctx) or b"").decode()


def _check(lib, st: int, ctx=None) -> None:
    if st != L.MBK_OK:
        raise MbkError(st, _error_text(lib, ctx))


def _out_array(out: Optional[np.ndarray], shape, dtype) -> np.ndarray:
    """`out`, or a new array: C-contiguous, of this dtype and of the shape's size."""
    if out is None:
        return np.empty(shape, dtype)
    assert out.dtype == dtype and out.size == int(np.prod(shape)) and out.flags.c_contiguous
    return out


def _wanted(shape, counts: Optional[np.ndarray], byts: Optional[np.ndarray]):
    """(MBK_WANT_* flags, counts pointer, bytes pointer) of the host outputs that are not None, each checked as _out_array does."""
    flags = (L.MBK_WANT_COUNTS if counts is not None else 0) | (L.MBK_WANT_BYTES if byts is not None else 0)
    return (flags, None if counts is None else _out_array(counts, shape, np.int32).ctypes.data,
            None if byts is None else _out_array(byts, shape, np.uint8).ctypes.data)


@dataclass(frozen=True)
class View:
    """width x height samples of [start_r, start_r+range_r] x [start_i, start_i+range_i], endpoints
    included (np.linspace semantics, WorkerCUDA.py:24-32)."""
    start_r: float
    start_i: float
    range_r: float
    range_i: float
    width: int
    height: int

    @staticmethod
    def centered(center_r: float, center_i: float, span: float, width: int, height: Optional[int] = None):
        height = width if height is None else height
        return View(center_r - span / 2, center_i - span / 2, span, span, width, height)


@dataclass(frozen=True)
class DeepView:
    """A deep-zoom view (include/mbk.h, "Deep-zoom views"): width x height pixels centred on a DeepOrbit's centre, spans
    span_r x span_i (end samples included).  span_i defaults to square pixels: span_r * (height-1) / (width-1)."""
    span_r: float
    width: int
    height: Optional[int] = None
    span_i: Optional[float] = None

    def __post_init__(self):
        h = self.width if self.height is None else int(self.height)
        object.__setattr__(self, "height", h)
        if self.span_i is None:
            si = self.span_r if (self.width <= 1 or h <= 1 or h == self.width) else self.span_r * (h - 1) / (self.width - 1)
            object.__setattr__(self, "span_i", float(si))


@dataclass(frozen=True)
class WideDeepView:
    """An extended-range deep view (include/mbk.h, "Extended-range deep views"): spans range_r 2^exp2 x range_i 2^exp2 with
    range_* in [2^-64, 4] and exp2 in [-8192, 0], so a span far below binary64's 1e-308 can be named.  range_i defaults to
    square pixels, as for DeepView."""
    range_r: float
    exp2: int
    width: int
    height: Optional[int] = None
    range_i: Optional[float] = None

    def __post_init__(self):
        h = self.width if self.height is None else int(self.height)
        object.__setattr__(self, "height", h)
        object.__setattr__(self, "exp2", int(self.exp2))
        if self.range_i is None:
            ri = self.range_r if (self.width <= 1 or h <= 1 or h == self.width) else self.range_r * (h - 1) / (self.width - 1)
            object.__setattr__(self, "range_i", float(ri))

    @staticmethod
    def from_decimal(span: Union[str, Decimal, Fraction, int, float], width: int, height: Optional[int] = None):
        """The view whose real span is the decimal `span` ("1e-600"): converted exactly, exp2 = floor(log2 span) clamped to [-8192, 0], and
        the mantissa span / 2^exp2 rounded once, to the nearest binary64."""
        f = Fraction(Decimal(span)) if isinstance(span, str) else Fraction(span)
        if f <= 0:
            raise ValueError("the span must be > 0")
        e = f.numerator.bit_length() - f.denominator.bit_length()      # floor(log2 f) is e or e - 1
        if Fraction(2) ** e > f:
            e -= 1
        exp2 = max(min(e, 0), -8192)
        return WideDeepView((f.numerator << -exp2) / f.denominator, exp2, width, height)

    @property
    def min_span_exp2(self) -> int:
        """floor(log2) of the smaller span: what DeepOrbit(min_span_exp2=...) takes."""
        return self.exp2 + math.frexp(min(self.range_r, self.range_i))[1] - 1


@dataclass(frozen=True)
class DensityTarget:
    """The target of a density view (include/mbk.h, "Density views"): the rectangle [start_r, start_r + range_r) x
    [start_i, start_i + range_i) cut into width x height half-open cells; the table is uint32[height, width], row 0 the
    lowest imaginary part."""
    start_r: float
    start_i: float
    range_r: float
    range_i: float
    width: int
    height: int

    def ctarget(self) -> L.mbk_density_target:
        return L.mbk_density_target(self.start_r, self.start_i, self.range_r, self.range_i, self.width, self.height)


@dataclass
class DensityStats:
    deposits: int   # orbit points that landed in a cell
    dropped: int    # orbit points of qualifying samples that fell outside the target


def _decimal_string(x, precision_bits: int) -> str:
    """An exact decimal for str / Decimal / int / float; for a Fraction with no finite decimal form, enough digits that
    the truncation to precision_bits fraction bits is the same as that of the Fraction itself."""
    if isinstance(x, str):
        return x.strip()
    if isinstance(x, bool):
        raise TypeError("a centre coordinate must be str, Decimal, Fraction, int or float")
    if isinstance(x, int):
        return str(x)
    if isinstance(x, float):
        return str(Decimal(x))   # exact; nan / inf are refused by the library's parser
    if isinstance(x, Decimal):
        return str(x)
    if isinstance(x, Fraction):
        num, den = abs(x.numerator), x.denominator
        d, a, b = den, 0, 0
        while d % 2 == 0:
            d, a = d // 2, a + 1
        while d % 5 == 0:
            d, b = d // 5, b + 1
        # terminating: exact.  Otherwise the fraction part of x * 2^P is >= 1/den, so 10^-k < 2^-P / den keeps the floor.
        k = max(a, b) if d == 1 else math.ceil(precision_bits * math.log10(2)) + len(str(den)) + 2
        q = str(num * 10 ** k // den).rjust(k + 1, "0")
        body = q[:-k] + "." + q[-k:] if k else q
        return ("-" if x < 0 else "") + body
    raise TypeError("a centre coordinate must be str, Decimal, Fraction, int or float")


def default_precision_bits(min_span: Optional[float], min_span_exp2: Optional[int] = None) -> int:
    """64 + ceil(-log2 min_span), rounded up to a multiple of 64 (min_span None: 2^-960, the deepest span a view takes).
    min_span_exp2: the span as a power of two, 2^min_span_exp2, for spans a float cannot hold (WideDeepView.min_span_exp2)."""
    if min_span_exp2 is not None:
        if min_span is not None:
            raise ValueError("give min_span or min_span_exp2, not both")
        return min(4096, max(64, -(-(64 + max(0, -int(min_span_exp2))) // 64) * 64))
    span = 2.0 ** -960 if min_span is None else float(min_span)
    if not (span > 0.0 and math.isfinite(span)):
        raise ValueError("min_span must be finite and > 0")
    bits = 64 + max(0, math.ceil(-math.log2(span)))
    return min(4096, max(64, -(-bits // 64) * 64))


class DeepOrbit:
    """The reference orbit of a deep view's centre (mbk_deep_orbit_*): computed on the host in fixed point with
    precision_bits fraction bits, up to mrd; needs no GPU.  Read-only; any MandelbrotDevice may use it."""

    def __init__(self, center_r: Union[str, Decimal, Fraction, int, float], center_i: Union[str, Decimal, Fraction, int, float],
                 mrd: int, *, min_span: Optional[float] = None, precision_bits: Optional[int] = None,
                 min_span_exp2: Optional[int] = None):
        self._lib = L.load()
        self._h = None
        bits = int(precision_bits) if precision_bits is not None else default_precision_bits(min_span, min_span_exp2)
        self.center = (_decimal_string(center_r, bits), _decimal_string(center_i, bits))
        h = C.c_void_p()
        st = self._lib.mbk_deep_orbit_create(self.center[0].encode(), self.center[1].encode(), bits, int(mrd), C.byref(h))
        _check(self._lib, st)
        self._h = h
        n, esc, p, m = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.mbk_deep_orbit_info(h, C.byref(n), C.byref(esc), C.byref(p), C.byref(m)))
        self.length, self.escaped, self.precision_bits, self.mrd = int(n.value), bool(esc.value), int(p.value), int(m.value)

    def _check(self, st: int) -> None:
        _check(self._lib, st)

    def table(self) -> Tuple[np.ndarray, np.ndarray]:
        """(Zr, Zi): Z_0 .. Z_M as float64."""
        zr = np.empty(self.length + 1, np.float64)
        zi = np.empty(self.length + 1, np.float64)
        self._check(self._lib.mbk_deep_orbit_read(self._h, zr.ctypes.data, zi.ctypes.data, zr.size))
        return zr, zi

    def wide_table(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(X_r float64, X_i float64, xe int32): Z_0 .. Z_M of the wide table, Z_m = X 2^xe (a zero Z: (0, 0, -2^24))."""
        xr = np.empty(self.length + 1, np.float64)
        xi = np.empty(self.length + 1, np.float64)
        xe = np.empty(self.length + 1, np.int32)
        self._check(self._lib.mbk_deep_orbit_read_wide(self._h, xr.ctypes.data, xi.ctypes.data, xe.ctypes.data, xr.size))
        return xr, xi, xe

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.mbk_deep_orbit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class TileStats:
    kernel_ms: float
    d2h_ms: float
    pixel_iterations: int
    never_pixels: int
    all_bytes_zero: bool   # DataChunk.IsNeverChunk (DataChunk.cs:82)
    all_bytes_one: bool    # DataChunk.IsImmediateChunk (DataChunk.cs:87)
    rle_runs: int = 0      # runs of equal bytes: RLE codec size = 1 + 5*rle_runs (DataChunkSerializer.cs:56-100)


def device_count() -> int:
    lib = L.load()
    n = C.c_int(0)
    st = lib.mbk_device_count(C.byref(n))
    if st != L.MBK_OK:
        return 0
    return n.value


def datachunk_geometry(level: int, index_real: int, index_imag: int) -> Tuple[float, float, float]:
    """(start_r, start_i, range) of a DataChunk tile: WorkerCUDA.py:75-78 == DataChunk.cs:32-33,59-66."""
    lib = L.load()
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    _check(lib, lib.mbk_datachunk_geometry(level, index_real, index_imag, C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def julia_count_host(z, c, mrd: int) -> Tuple[int, float]:
    """mbk_julia_count_host: (n, mag) of one Julia orbit -- z -> z^2 + c from z_0 = z -- on the host, without a device: the
    contract's loop (include/mbk.h, "Julia views") with the doubling a launch with this c would use."""
    lib = L.load()
    n, mag = C.c_int32(0), C.c_double(0.0)
    _check(lib, lib.mbk_julia_count_host(float(z[0]), float(z[1]), float(c[0]), float(c[1]), mrd, C.byref(n), C.byref(mag)))
    return int(n.value), float(mag.value)


def julia_distance_host(z, c, mrd: int) -> dict:
    """mbk_julia_distance_host: one Julia orbit with its derivative dz_k/dz_0 on the host, without a device, compiled from the
    step function the kernels use (include/mbk.h, "Distance estimates for Julia views"): a dict of the final state -- n, extra
    (the run-on steps taken), zr, zi, dr, di, mag, dmag and de (through the host's ln)."""
    lib = L.load()
    n, x = C.c_int32(0), C.c_int32(0)
    vals = [C.c_double(0.0) for _ in range(7)]
    _check(lib, lib.mbk_julia_distance_host(float(z[0]), float(z[1]), float(c[0]), float(c[1]), mrd, C.byref(n), C.byref(x),
                                            *[C.byref(v) for v in vals]))
    out = {"n": int(n.value), "extra": int(x.value)}
    out.update((k, float(v.value)) for k, v in zip(("zr", "zi", "dr", "di", "mag", "dmag", "de"), vals))
    return out


def _cxview(view: "WideDeepView", window=None) -> L.mbk_deep_xview:
    col0, row0, ncols, nrows = window if window is not None else (0, 0, view.width, view.height)
    return L.mbk_deep_xview(view.range_r, view.range_i, view.exp2, view.width, view.height, col0, row0, ncols, nrows)


def deep_xbla_table(orbit: "DeepOrbit", view: "WideDeepView", window=None) -> list:
    """mbk_deep_xbla_info / _read: the table an xbla=True launch of `view` on `orbit` would use (include/mbk.h, "Extended-range
    deep views with bilinear approximation"), built on the host, without a device.  A list of levels, each a dict of arrays:
    Ar, Ai (float64), ae (int32), Br, Bi (float64), be, ke (int32); [] for an orbit of length 1.  The window plays no part."""
    lib = L.load()
    cv = _cxview(view, window)
    levels, entries = C.c_uint32(), C.c_uint64()
    _check(lib, lib.mbk_deep_xbla_info(orbit._h, C.byref(cv), C.byref(levels), C.byref(entries)))
    out = []
    for l in range(levels.value):
        n = (orbit.length - 1) >> l
        lv = {k: np.empty(n, np.float64 if k[0] in "AB" else np.int32) for k in ("Ar", "Ai", "ae", "Br", "Bi", "be", "ke")}
        _check(lib, lib.mbk_deep_xbla_read(orbit._h, C.byref(cv), l, *[a.ctypes.data for a in lv.values()], n))
        out.append(lv)
    assert sum(lv["ke"].size for lv in out) == entries.value
    return out


def deep_xbla_count_host(orbit: "DeepOrbit", view: "WideDeepView", pixels, mrd: int, window=None):
    """mbk_deep_xbla_count_host on the pixels (row-major indices of the FULL view): (count int32, mag float64, steps executed
    int64 -- a skip is one) per pixel, on the host, from the functions the kernel uses."""
    lib = L.load()
    cv = _cxview(view, window)
    pixels = np.asarray(pixels, np.int64).ravel()
    count, mag, steps = np.empty(pixels.size, np.int32), np.empty(pixels.size, np.float64), np.empty(pixels.size, np.int64)
    c, m, s = C.c_int32(), C.c_double(), C.c_uint64()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_xbla_count_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                                 C.byref(c), C.byref(m), C.byref(s)))
        count[j], mag[j], steps[j] = c.value, m.value, s.value
    return count, mag, steps


def wide_distance_host(orbit: "DeepOrbit", view: "WideDeepView", pixels, mrd: int) -> dict:
    """mbk_deep_xview_distance_host on the pixels (row-major indices of the FULL view), on the host, from the functions the
    kernel uses (include/mbk.h, "Distance estimates for extended-range deep views"): a dict of arrays n (int32), extra (the
    run-on steps taken, int32), mag, Dr, Di (float64), e (int64: d = D 2^e), dmagD and rel (float64, through the host's ln)."""
    lib = L.load()
    cv = _cxview(view)
    pixels = np.asarray(pixels, np.int64).ravel()
    out = {k: np.empty(pixels.size, t) for k, t in (("n", np.int32), ("extra", np.int32), ("mag", np.float64), ("Dr", np.float64),
                                                   ("Di", np.float64), ("e", np.int64), ("rel", np.float64))}
    n, x, e = C.c_int32(), C.c_int32(), C.c_int32()
    mag, dr, di, rel = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_xview_distance_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                                     C.byref(n), C.byref(x), C.byref(mag), C.byref(dr), C.byref(di), C.byref(e),
                                                     C.byref(rel)))
        for key, v in (("n", n), ("extra", x), ("mag", mag), ("Dr", dr), ("Di", di), ("e", e), ("rel", rel)):
            out[key][j] = v.value
    a = out["Dr"] * out["Dr"]
    b = out["Di"] * out["Di"]
    out["dmagD"] = a + b
    return out


def wide_distance_step_host(z_r: float, z_i: float, t: int, D_r: float, D_i: float, e: int) -> Tuple[float, float, int]:
    """mbk_deep_xdistance_step_host: one derivative step d' = 2 zp d + 1 on zp = (z_r, z_i) 2^t and d = (D_r, D_i) 2^e;
    returns the new (D_r, D_i, e)."""
    lib = L.load()
    dr, di, ce = C.c_double(float(D_r)), C.c_double(float(D_i)), C.c_int32(int(e))
    _check(lib, lib.mbk_deep_xdistance_step_host(float(z_r), float(z_i), int(t), C.byref(dr), C.byref(di), C.byref(ce)))
    return float(dr.value), float(di.value), int(ce.value)


def wide_distance_value_host(mag: float, dmagD: float, e: int, range_r: float, exp2: int, count: int) -> float:
    """mbk_deep_xdistance_value_host: the output rule rel = de / (range_r 2^exp2) on the host (with the host's ln)."""
    return float(L.load().mbk_deep_xdistance_value_host(float(mag), float(dmagD), int(e), float(range_r), int(exp2), int(count)))


def wide_distance_xbla_host(orbit: "DeepOrbit", view: "WideDeepView", pixels, mrd: int, window=None) -> dict:
    """mbk_deep_xview_distance_xbla_host on the pixels (row-major indices of the FULL view), on the host, from the functions the
    kernel uses (include/mbk.h, "Distance estimates for extended-range deep views with bilinear approximation"): a dict of
    arrays n (int32), extra (the run-on steps taken, int32), mag, Dr, Di (float64), e (int64: d = D 2^e), dmagD and rel
    (float64, through the host's ln) and steps (int64: the steps executed in the count loop, a skip counting as one).  A
    window changes nothing: the table is the full view's."""
    lib = L.load()
    cv = _cxview(view, window)
    pixels = np.asarray(pixels, np.int64).ravel()
    out = {k: np.empty(pixels.size, t) for k, t in (("n", np.int32), ("extra", np.int32), ("mag", np.float64), ("Dr", np.float64),
                                                   ("Di", np.float64), ("e", np.int64), ("rel", np.float64), ("steps", np.int64))}
    n, x, e, s = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    mag, dr, di, rel = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_xview_distance_xbla_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                                          C.byref(n), C.byref(x), C.byref(mag), C.byref(dr), C.byref(di),
                                                          C.byref(e), C.byref(rel), C.byref(s)))
        for key, v in (("n", n), ("extra", x), ("mag", mag), ("Dr", dr), ("Di", di), ("e", e), ("rel", rel), ("steps", s)):
            out[key][j] = v.value
    a = out["Dr"] * out["Dr"]
    b = out["Di"] * out["Di"]
    out["dmagD"] = a + b
    return out


def wide_distance_xbla_skip_host(A_r: float, A_i: float, a_e: int, B_r: float, B_i: float, b_e: int, D_r: float, D_i: float,
                                 e: int) -> Tuple[float, float, int]:
    """mbk_deep_xdistance_skip_host: the derivative across one skip, d' = A d + B on A = (A_r, A_i) 2^a_e, B = (B_r, B_i) 2^b_e
    and d = (D_r, D_i) 2^e; returns the new (D_r, D_i, e)."""
    lib = L.load()
    dr, di, ce = C.c_double(float(D_r)), C.c_double(float(D_i)), C.c_int32(int(e))
    _check(lib, lib.mbk_deep_xdistance_skip_host(float(A_r), float(A_i), int(a_e), float(B_r), float(B_i), int(b_e), C.byref(dr),
                                                 C.byref(di), C.byref(ce)))
    return float(dr.value), float(di.value), int(ce.value)


def deep_distance_bla_host(orbit: "DeepOrbit", view: "DeepView", pixels, mrd: int) -> dict:
    """mbk_deep_distance_bla_host on the pixels (row-major indices of the FULL view), on the host, from the functions the kernel
    uses (include/mbk.h, "Distance estimates for deep views with bilinear approximation"): a dict of arrays n (int32), extra
    (the run-on steps taken, int32), mag, Dr, Di (float64), e (int64: d = D 2^e), dmagD and rel (float64, through the host's
    ln) and steps (int64: the steps executed in the count loop, a skip counting as one)."""
    lib = L.load()
    cv = L.mbk_deep_view(view.span_r, view.span_i, view.width, view.height, 0, 0, view.width, view.height)
    pixels = np.asarray(pixels, np.int64).ravel()
    out = {k: np.empty(pixels.size, t) for k, t in (("n", np.int32), ("extra", np.int32), ("mag", np.float64), ("Dr", np.float64),
                                                   ("Di", np.float64), ("e", np.int64), ("rel", np.float64), ("steps", np.int64))}
    n, x, e, s = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    mag, dr, di, rel = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_distance_bla_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                                   C.byref(n), C.byref(x), C.byref(mag), C.byref(dr), C.byref(di), C.byref(e),
                                                   C.byref(rel), C.byref(s)))
        for key, v in (("n", n), ("extra", x), ("mag", mag), ("Dr", dr), ("Di", di), ("e", e), ("rel", rel), ("steps", s)):
            out[key][j] = v.value
    a = out["Dr"] * out["Dr"]
    b = out["Di"] * out["Di"]
    out["dmagD"] = a + b
    return out


def deep_distance_bla_skip_host(A_r: float, A_i: float, B_r: float, B_i: float, D_r: float, D_i: float, e: int) -> Tuple[float, float, int]:
    """mbk_deep_distance_bla_skip_host: the derivative across one skip, d' = A d + B on d = (D_r, D_i) 2^e; returns the new
    (D_r, D_i, e)."""
    lib = L.load()
    dr, di, ce = C.c_double(float(D_r)), C.c_double(float(D_i)), C.c_int32(int(e))
    _check(lib, lib.mbk_deep_distance_bla_skip_host(float(A_r), float(A_i), float(B_r), float(B_i), C.byref(dr), C.byref(di), C.byref(ce)))
    return float(dr.value), float(di.value), int(ce.value)


def _no_wide_relief(view) -> None:
    if not isinstance(view, DeepView):
        raise MbkError(L.MBK_ERR_INVALID, "relief shading is implemented for a DeepView only: a WideDeepView (spans below 2^-960) "
                                          "takes compute_wide_view_normals / render_wide_view_relief / wide_normal_host")


def _wide_relief_only(view, name: str, deep_name: str) -> None:
    if not isinstance(view, WideDeepView):
        raise ValueError(f"{name} takes a WideDeepView (a DeepView: {deep_name})")


def deep_normal_host(orbit: "DeepOrbit", view: "DeepView", pixels, mrd: int, bla: bool = False) -> dict:
    """mbk_deep_normal_host on the pixels (row-major indices of the FULL view), on the host, from the functions the kernels use
    (include/mbk.h, "Relief shading for deep views"): a dict of arrays n (int32), extra (the run-on steps taken, int32), zpr,
    zpi, Dr, Di (float64: the final z and the derivative D 2^e), e (int64), normal (float64[k, 2]), nu (float64, through the
    host's logarithms) and steps (int64: the steps executed in the count loop, a skip counting as one)."""
    _no_wide_relief(view)
    lib = L.load()
    cv = L.mbk_deep_view(view.span_r, view.span_i, view.width, view.height, 0, 0, view.width, view.height)
    pixels = np.asarray(pixels, np.int64).ravel()
    out = {k: np.empty(pixels.size, t) for k, t in (("n", np.int32), ("extra", np.int32), ("zpr", np.float64), ("zpi", np.float64),
                                                   ("Dr", np.float64), ("Di", np.float64), ("e", np.int64), ("nu", np.float64),
                                                   ("steps", np.int64))}
    out["normal"] = np.empty((pixels.size, 2), np.float64)
    n, x, e, s = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    zr, zi, dr, di, nu = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
    nrm = (C.c_double * 2)()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_normal_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                             L.MBK_DEEP_BLA if bla else 0, C.byref(n), C.byref(x), C.byref(zr), C.byref(zi),
                                             C.byref(dr), C.byref(di), C.byref(e), nrm, C.byref(nu), C.byref(s)))
        for key, v in (("n", n), ("extra", x), ("zpr", zr), ("zpi", zi), ("Dr", dr), ("Di", di), ("e", e), ("nu", nu), ("steps", s)):
            out[key][j] = v.value
        out["normal"][j] = nrm[0], nrm[1]
    return out


def wide_normal_host(orbit: "DeepOrbit", view: "WideDeepView", pixels, mrd: int, xbla: bool = False, window=None) -> dict:
    """mbk_deep_xview_normal_host on the pixels (row-major indices of the FULL view), on the host, from the functions the
    kernels use (include/mbk.h, "Relief shading for extended-range deep views"): the dict of deep_normal_host -- zpr, zpi the
    mantissas of the final z -- plus t (int64: z = (zpr, zpi) 2^t; d = (Dr, Di) 2^e).  A window changes nothing: the table of
    xbla is the full view's."""
    _wide_relief_only(view, "wide_normal_host", "deep_normal_host")
    lib = L.load()
    cv = _cxview(view, window)
    pixels = np.asarray(pixels, np.int64).ravel()
    out = {k: np.empty(pixels.size, t) for k, t in (("n", np.int32), ("extra", np.int32), ("zpr", np.float64), ("zpi", np.float64),
                                                   ("t", np.int64), ("Dr", np.float64), ("Di", np.float64), ("e", np.int64),
                                                   ("nu", np.float64), ("steps", np.int64))}
    out["normal"] = np.empty((pixels.size, 2), np.float64)
    n, x, t, e, s = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    zr, zi, dr, di, nu = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
    nrm = (C.c_double * 2)()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_xview_normal_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                                   L.MBK_DEEP_XBLA if xbla else 0, C.byref(n), C.byref(x), C.byref(zr), C.byref(zi),
                                                   C.byref(t), C.byref(dr), C.byref(di), C.byref(e), nrm, C.byref(nu), C.byref(s)))
        for key, v in (("n", n), ("extra", x), ("zpr", zr), ("zpi", zi), ("t", t), ("Dr", dr), ("Di", di), ("e", e), ("nu", nu),
                       ("steps", s)):
            out[key][j] = v.value
        out["normal"][j] = nrm[0], nrm[1]
    return out


# -- locating minibrots (include/mbk.h, "Locating minibrots in deep views") ---------------------------------------------------

class NucleusError(RuntimeError):
    """refine_nucleus / locate_nucleus could not deliver a nucleus; `reason` is "no seed", "not converged" or "precision"."""

    def __init__(self, reason: str, message: str):
        super().__init__(f"{reason}: {message}")
        self.reason = reason


def _big_int(digits: str) -> int:
    """int(digits) for a string of decimal digits of any length (int() refuses more than a few thousand at once)."""
    v = 0
    for k in range(0, len(digits), 1000):
        part = digits[k:k + 1000]
        v = v * 10 ** len(part) + int(part)
    return v


def _big_str(v: int) -> str:
    """str(v) for a non-negative int of any size."""
    parts = []
    while True:
        v, low = divmod(v, 10 ** 1000)
        if v == 0:
            parts.append(str(low))
            break
        parts.append(str(low).rjust(1000, "0"))
    return "".join(reversed(parts))


def _exact_fraction(x) -> Fraction:
    """The exact value of a centre coordinate (str in the library's decimal syntax, Decimal, Fraction, int or float)."""
    if isinstance(x, Fraction):
        return x
    if isinstance(x, (int, float)) and not isinstance(x, bool):
        return Fraction(x)
    s = str(x).strip().lower()
    neg = s.startswith("-")
    if s[:1] in "+-":
        s = s[1:]
    mant, _, ex = s.partition("e")
    whole, _, frac = mant.partition(".")
    if not (whole + frac).isdigit():
        raise ValueError(f"not a decimal number: {x!r}")
    e10 = (int(ex) if ex else 0) - len(frac)
    v = Fraction(_big_int(whole + frac)) * (Fraction(10) ** e10)
    return -v if neg else v


def _dyadic_decimal(x: Fraction) -> str:
    """The exact decimal string of a Fraction whose denominator is a power of two."""
    k = x.denominator.bit_length() - 1
    if x.denominator != 1 << k:
        raise ValueError("not a dyadic fraction")
    q = _big_str(abs(x.numerator) * 5 ** k).rjust(k + 1, "0")
    body = q[:-k] + "." + q[-k:] if k else q
    return ("-" if x < 0 else "") + body


def _wide_fraction(m: float, e: int) -> Fraction:
    """m 2^e exactly (a wide zero, exponent -2^24, is 0)."""
    if m == 0.0:
        return Fraction(0)
    if not math.isfinite(m):
        raise NucleusError("not converged", "a non-finite value")
    return Fraction(m) * (Fraction(2) ** int(e))


def deep_nucleus_host(orbit: "DeepOrbit", view: "DeepView", pixels, mrd: int) -> dict:
    """mbk_deep_nucleus_host on the pixels (row-major indices of the FULL view), on the host, from the functions the kernel uses
    (include/mbk.h, "Locating minibrots in deep views"): a dict of arrays n, period (int32), best (float64), z (float64[N, 2]),
    D (float64[N, 2]), e (int64: d_b = D 2^e) and delta (float64[N, 2])."""
    lib = L.load()
    if not isinstance(view, DeepView):
        raise ValueError("atom periods are implemented for a DeepView only")
    cv = L.mbk_deep_view(view.span_r, view.span_i, view.width, view.height, 0, 0, view.width, view.height)
    pixels = np.asarray(pixels, np.int64).ravel()
    N = pixels.size
    out = {"n": np.empty(N, np.int32), "period": np.empty(N, np.int32), "best": np.empty(N, np.float64),
           "z": np.empty((N, 2), np.float64), "D": np.empty((N, 2), np.float64), "e": np.empty(N, np.int64),
           "delta": np.empty((N, 2), np.float64)}
    n, p, e, best = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    z, d, delta = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_nucleus_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                              C.byref(n), C.byref(p), C.byref(best), z, d, C.byref(e), delta))
        out["n"][j], out["period"][j], out["best"][j], out["e"][j] = n.value, p.value, best.value, e.value
        out["z"][j], out["D"][j], out["delta"][j] = tuple(z), tuple(d), tuple(delta)
    return out


def _orbit_wide_call(name: str, orbit: "DeepOrbit", period: int) -> Tuple[float, float, int]:
    lib = L.load()
    r, i, e = C.c_double(), C.c_double(), C.c_int32()
    _check(lib, getattr(lib, name)(orbit._h, int(period), C.byref(r), C.byref(i), C.byref(e)))
    return float(r.value), float(i.value), int(e.value)


def orbit_newton_host(orbit: "DeepOrbit", period: int) -> Tuple[float, float, int]:
    """mbk_deep_orbit_newton_host: the Newton step -Z_p / D_p at the orbit's own centre as (d_r, d_i, d_e), value d 2^d_e."""
    return _orbit_wide_call("mbk_deep_orbit_newton_host", orbit, period)


def orbit_size_host(orbit: "DeepOrbit", period: int) -> Tuple[float, float, int]:
    """mbk_deep_orbit_size_host: the size estimate 1 / (b l^2) of the component whose nucleus the orbit's centre is, as
    (s_r, s_i, s_e), value s 2^s_e."""
    return _orbit_wide_call("mbk_deep_orbit_size_host", orbit, period)


def _pixel_offsets(view: "DeepView"):
    """(dc_r[width], dc_i[height]): the offsets of the view's columns and rows as the kernels form them."""
    def axis(n, span):
        if n <= 1:
            return np.zeros(n, np.float64)
        return (np.arange(n, dtype=np.float64) - np.float64((n - 1) / 2)) * (np.float64(span) / np.float64(n - 1))
    return axis(view.width, view.span_r), axis(view.height, view.span_i)


class NucleusSeed(NamedTuple):
    pixel: Tuple[int, int]   # (row, col)
    period: int
    offset_r: Fraction       # the target, from the view's centre, in the plane's units
    offset_i: Fraction


def pick_nucleus_seed(view: "DeepView", period, delta) -> Optional[NucleusSeed]:
    """The Newton seed of a view from the outputs of compute_deep_view_nucleus (period int32[height, width], delta
    float64[height, width, 2]).  The target of a pixel is its offset plus delta * span_r, exactly (Fractions); it is in view
    when it lies within the view's rectangle.  Among the in-view pixels with a finite delta the lowest period wins, among those
    the smallest |delta|, among those the first in image order.  None when no target is in view."""
    return _pick_seed(view.width, view.height, view.span_r, view.span_i, Fraction(1), period, delta)


def _pick_seed(width: int, height: int, range_r: float, range_i: float, unit: Fraction, period, delta) -> Optional[NucleusSeed]:
    """pick_nucleus_seed's rule on a view of spans range_r unit x range_i unit (unit 1: a DeepView; 2^exp2: a WideDeepView).
    Every decision is taken in units of `unit` -- the float pre-test on the offsets and delta * range_r as binary64, the exact
    one on Fractions -- so nothing is ever multiplied by the unit in binary64; only the offsets returned carry it."""
    period = np.asarray(period)
    delta = np.asarray(delta, np.float64).reshape(height, width, 2)
    assert period.shape == (height, width)
    dcr, dci = _pixel_offsets(DeepView(range_r, width, height, range_i))
    span_r, span_i = Fraction(range_r), Fraction(range_i)
    finite = np.isfinite(delta).all(axis=2)
    with np.errstate(all="ignore"):
        tr = dcr[None, :] + delta[..., 0] * range_r
        ti = dci[:, None] + delta[..., 1] * range_r
        # the float test decides all but the targets within 1e-12 (relative) of an edge; those are decided exactly
        near = 1e-12
        surely_in = finite & (np.abs(tr) <= range_r / 2 * (1 - near)) & (np.abs(ti) <= range_i / 2 * (1 - near))
        maybe_in = finite & (np.abs(tr) <= range_r / 2 * (1 + near)) & (np.abs(ti) <= range_i / 2 * (1 + near))
        mag2 = delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]

    def target(r, c):
        return (Fraction(float(dcr[c])) + Fraction(float(delta[r, c, 0])) * span_r,
                Fraction(float(dci[r])) + Fraction(float(delta[r, c, 1])) * span_r)

    def in_view(r, c):
        if surely_in[r, c]:
            return True
        t = target(r, c)
        return abs(t[0]) * 2 <= span_r and abs(t[1]) * 2 <= span_i

    for p in np.unique(period[maybe_in]):
        cand = [(r, c) for r, c in zip(*np.nonzero(maybe_in & (period == p))) if in_view(r, c)]
        if not cand:
            continue
        low = min(mag2[r, c] for r, c in cand)
        close = [(r, c) for r, c in cand if mag2[r, c] <= low * (1 + near)]
        exact = lambda rc: Fraction(float(delta[rc[0], rc[1], 0])) ** 2 + Fraction(float(delta[rc[0], rc[1], 1])) ** 2
        r, c = min(close, key=exact)   # (min keeps the first of equals: image order)
        t = target(r, c)
        return NucleusSeed((int(r), int(c)), int(p), t[0] * unit, t[1] * unit)
    return None


@dataclass(frozen=True)
class Nucleus:
    """A located minibrot: its nucleus as decimal strings (found at precision_bits fraction bits, then polished at more: see
    refine_nucleus), its minimal period and the
    size estimate (size_r, size_i) 2^size_e of its component (complex: its argument is the minibrot's orientation)."""
    center_r: str
    center_i: str
    period: int
    size_r: float
    size_i: float
    size_e: int
    precision_bits: int
    rounds: int
    polish_rounds: int = 0   # further rounds at a higher precision: the centre strings carry more than precision_bits
    seed_pixel: Optional[Tuple[int, int]] = None
    inside: Optional[bool] = None

    @property
    def size_log2(self) -> float:
        """log2 |size|"""
        return self.size_e + math.log2(math.hypot(self.size_r, self.size_i))

    def orbit(self, mrd: int) -> "DeepOrbit":
        """The reference orbit of the nucleus at precision_bits."""
        return DeepOrbit(self.center_r, self.center_i, mrd, precision_bits=self.precision_bits)

    def view(self, width: int, height: Optional[int] = None, frame: float = 4.0):
        """The view centred on the nucleus whose real span is frame * |size|: a DeepView, or a WideDeepView when that span is
        below 2^-960."""
        f, k = math.frexp(float(frame) * math.hypot(self.size_r, self.size_i))
        if self.size_e + k - 1 < -960:
            return WideDeepView(f, self.size_e + k, width, height)
        return DeepView(min(4.0, math.ldexp(f, self.size_e + k)), width, height)


def refine_nucleus(center_r, center_i, period: int, precision_bits: int, max_rounds: int = 32) -> Nucleus:
    """Newton's method on Z_p(C) = 0 from the seed (center_r, center_i), on the host.  Each round builds the reference orbit of
    C at precision_bits fraction bits, takes the step -Z_p / D_p (mbk_deep_orbit_newton_host) and adds it to C exactly; it has
    converged when |step| <= 2^(32 - precision_bits) (the fixed-point orbit's truncation noise in Z_p / D_p is of the order of
    p 2^-precision_bits).  The period is then reduced to the smallest divisor of `period` whose own Newton step at the result
    meets the same bound, and the size estimate is taken.  Last, the centre is polished: Z_p(C) = D_p (C - root) with |D_p| about
    1 / sqrt(size), so a centre good to its last place at precision_bits still leaves Z_p far above 2^-precision_bits; the same
    rounds at precision_bits + log2(1 / sqrt(size)) + 64 bits (at most 4096) go on until |Z_p| <= 2^(38 - precision_bits), and the
    centre strings returned carry those bits (Nucleus.orbit reads precision_bits of them; a later, deeper orbit may read more).
    Raises NucleusError: "not converged" (max_rounds used up in either phase, or the
    iterate left the set's neighbourhood), or "precision" (-log2 |size| + 64 > precision_bits: the component is too small for
    this precision to place a view in it)."""
    period, P = int(period), int(precision_bits)
    if period < 1:
        raise ValueError("period must be >= 1")
    bound2 = Fraction(4) ** (32 - P)

    def truncated(v):
        """what the library reads of v: truncated towards zero at P fraction bits"""
        v = _exact_fraction(v)
        t = Fraction((abs(v.numerator) << P) // v.denominator, 1 << P)
        return -t if v < 0 else t

    Cr, Ci = truncated(center_r), truncated(center_i)   # (dyadic from here on: every sum below is exact and has a finite decimal)

    def step_at(cr, ci, q):
        """(orbit, the Newton step of period q at (cr, ci) as two Fractions)"""
        try:
            o = DeepOrbit(_dyadic_decimal(cr), _dyadic_decimal(ci), period + 1, precision_bits=P)
            d = orbit_newton_host(o, q)
        except MbkError as err:
            raise NucleusError("not converged", f"no Newton step of period {q} at the iterate ({err})") from None
        return o, _wide_fraction(d[0], d[2]), _wide_fraction(d[1], d[2])

    rounds = 0
    while True:
        if rounds == max_rounds:
            raise NucleusError("not converged", f"|step| is still above 2^{32 - P} after {max_rounds} rounds")
        _, dr, di = step_at(Cr, Ci, period)
        Cr, Ci = Cr + dr, Ci + di
        rounds += 1
        if dr * dr + di * di <= bound2:
            break
    Cr, Ci = truncated(Cr), truncated(Ci)
    o, _, _ = step_at(Cr, Ci, period)
    minimal = period
    for q in range(1, period):
        if period % q == 0:
            d = orbit_newton_host(o, q)
            qr, qi = _wide_fraction(d[0], d[2]), _wide_fraction(d[1], d[2])
            if qr * qr + qi * qi <= bound2:
                minimal = q
                break
    s = orbit_size_host(o, minimal)
    mag = math.hypot(s[0], s[1])
    if not (math.isfinite(mag) and mag > 0.0):
        raise NucleusError("not converged", "the size estimate is not finite")
    need = -(s[2] + math.log2(mag)) + 64
    if need > P:
        raise NucleusError("precision", f"the component has size 2^{s[2] + math.log2(mag):.1f}: {math.ceil(need)} fraction bits "
                                        f"are needed, precision_bits is {P}")
    # Polish.  C is now within 2^(32 - P) of the root, but Z_p(C) = D_p (C - root) and |D_p| = |b l| ~ 1 / sqrt(size) of a deep
    # minibrot is huge: a last-place error of C leaves Z_p far above 2^-P.  The same Newton rounds at Q = P + log2(1 / sqrt(size))
    # + 64 bits (a multiple of 64, at most 4096) go on until Z_p itself is below 2^(38 - P); the centre strings carry Q bits.
    Q = min(4096, -(-(P + math.ceil(need - 64) // 2 + 64) // 64) * 64)
    polish = 0
    while Q > P:
        try:
            o = DeepOrbit(_dyadic_decimal(Cr), _dyadic_decimal(Ci), minimal + 1, precision_bits=Q)
            d = orbit_newton_host(o, minimal)
        except MbkError as err:
            raise NucleusError("not converged", f"no Newton step at the polished iterate ({err})") from None
        xr, xi, xe = (a[minimal] for a in o.wide_table())
        z = (_wide_fraction(float(xr), int(xe)), _wide_fraction(float(xi), int(xe)))
        dr, di = _wide_fraction(d[0], d[2]), _wide_fraction(d[1], d[2])
        if z[0] * z[0] + z[1] * z[1] <= Fraction(4) ** (38 - P) or dr * dr + di * di <= Fraction(4) ** (32 - Q):
            break
        if polish == max_rounds:
            raise NucleusError("not converged", f"|Z_p| is still above 2^{38 - P} after {max_rounds} polishing rounds at {Q} bits")
        Cr, Ci = Cr + dr, Ci + di
        t = [Fraction((abs(v.numerator) << Q) // v.denominator, 1 << Q) * (-1 if v < 0 else 1) for v in (Cr, Ci)]
        Cr, Ci = t
        polish += 1
    return Nucleus(_dyadic_decimal(Cr), _dyadic_decimal(Ci), minimal, s[0], s[1], s[2], P, rounds, polish)


def nucleus_precision_bits(view: "DeepView") -> int:
    """locate_nucleus' default precision: the next multiple of 64 at or above 2 log2(1 / span) + 128, at most 4096 -- the sizes
    found in a view are about its span squared."""
    span = min(view.span_r, view.span_i)
    bits = math.ceil(2 * max(0.0, -math.log2(span)) + 128)
    return min(4096, -(-bits // 64) * 64)


def locate_nucleus(orbit: "DeepOrbit", view: "DeepView", mrd: int, *, seeds, precision_bits: Optional[int] = None,
                   max_rounds: int = 32) -> Nucleus:
    """The minibrot a view points at, from the view's atom periods and Newton seeds: seeds = (period, delta) as
    compute_deep_view_nucleus (or deep_nucleus_host over every pixel) gives them.  pick_nucleus_seed chooses the seed,
    refine_nucleus refines it at precision_bits (default nucleus_precision_bits(view)).  Host only;
    MandelbrotDevice.locate_nucleus computes the seeds on the device and calls this.  Raises NucleusError ("no seed": no
    target lies in the view)."""
    if not isinstance(view, DeepView):
        raise ValueError("locating a nucleus is implemented for a DeepView only")
    period, delta = seeds
    seed = pick_nucleus_seed(view, period, delta)
    if seed is None:
        raise NucleusError("no seed", f"no pixel's Newton target lies in the view at mrd {mrd}")
    P = int(precision_bits) if precision_bits is not None else nucleus_precision_bits(view)
    C0 = (_exact_fraction(orbit.center[0]), _exact_fraction(orbit.center[1]))
    n = refine_nucleus(C0[0] + seed.offset_r, C0[1] + seed.offset_i, seed.period, P, max_rounds)
    off = (_exact_fraction(n.center_r) - C0[0], _exact_fraction(n.center_i) - C0[1])
    inside = abs(off[0]) * 2 <= Fraction(view.span_r) and abs(off[1]) * 2 <= Fraction(view.span_i)
    return replace(n, seed_pixel=seed.pixel, inside=bool(inside))


# -- the same from extended-range views (include/mbk.h, "Locating minibrots in extended-range deep views") ---------------------

def wide_nucleus_host(orbit: "DeepOrbit", view: "WideDeepView", pixels, mrd: int) -> dict:
    """mbk_deep_xview_nucleus_host on the pixels (row-major indices of the FULL view), on the host, from the functions the kernel
    uses: a dict of arrays n, period (int32), best_m (float64) and best_e (int64: the normalised |z_b|^2 = best_m 2^best_e),
    z (float64[N, 2]) and t (int64: z_b = z 2^t), D (float64[N, 2]) and e (int64: d_b = D 2^e), and delta (float64[N, 2])."""
    lib = L.load()
    if not isinstance(view, WideDeepView):
        raise ValueError("wide_nucleus_host takes a WideDeepView (a DeepView: deep_nucleus_host)")
    cv = _cxview(view)
    pixels = np.asarray(pixels, np.int64).ravel()
    N = pixels.size
    out = {"n": np.empty(N, np.int32), "period": np.empty(N, np.int32), "best_m": np.empty(N, np.float64),
           "best_e": np.empty(N, np.int64), "z": np.empty((N, 2), np.float64), "t": np.empty(N, np.int64),
           "D": np.empty((N, 2), np.float64), "e": np.empty(N, np.int64), "delta": np.empty((N, 2), np.float64)}
    n, p, be, t, e, bm = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    z, d, delta = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 2)()
    for j, k in enumerate(pixels):
        _check(lib, lib.mbk_deep_xview_nucleus_host(orbit._h, C.byref(cv), int(k % view.width), int(k // view.width), int(mrd),
                                                    C.byref(n), C.byref(p), C.byref(bm), C.byref(be), z, C.byref(t), d, C.byref(e),
                                                    delta))
        out["n"][j], out["period"][j], out["best_m"][j], out["best_e"][j] = n.value, p.value, bm.value, be.value
        out["t"][j], out["e"][j] = t.value, e.value
        out["z"][j], out["D"][j], out["delta"][j] = tuple(z), tuple(d), tuple(delta)
    return out


def pick_wide_nucleus_seed(view: "WideDeepView", period, delta) -> Optional[NucleusSeed]:
    """pick_nucleus_seed for a WideDeepView, from the outputs of compute_wide_view_nucleus: the lowest period whose target is in
    view, then the smallest |delta|, then image order.  The target of a pixel is its offset plus delta * range_r in units of
    2^exp2; the float pre-test and the exact decision both work in those units, and only the offsets returned -- Fractions in
    the plane's units -- carry the 2^exp2, which binary64 cannot hold."""
    if not isinstance(view, WideDeepView):
        raise ValueError("pick_wide_nucleus_seed takes a WideDeepView (a DeepView: pick_nucleus_seed)")
    return _pick_seed(view.width, view.height, view.range_r, view.range_i, Fraction(2) ** view.exp2, period, delta)


def wide_nucleus_precision_bits(view: "WideDeepView") -> int:
    """locate_wide_nucleus' default precision: the next multiple of 64 at or above 2 * (-view.min_span_exp2) + 128, at most
    4096 -- the sizes found in a view are about its span squared."""
    bits = 2 * max(0, -view.min_span_exp2) + 128
    return min(4096, -(-bits // 64) * 64)


def locate_wide_nucleus(orbit: "DeepOrbit", view: "WideDeepView", mrd: int, *, seeds, precision_bits: Optional[int] = None,
                        max_rounds: Optional[int] = None) -> Nucleus:
    """locate_nucleus for a WideDeepView: seeds = (period, delta) as compute_wide_view_nucleus (or wide_nucleus_host over every
    pixel) gives them, pick_wide_nucleus_seed chooses the seed, refine_nucleus refines it at precision_bits (default
    wide_nucleus_precision_bits(view)).  max_rounds None: max(32, ceil(precision_bits / 40)) -- a binary64 Newton step gains
    about 51 bits a round, so a seed good to the view's span needs about precision_bits / 51 rounds.  Host only;
    MandelbrotDevice.locate_wide_nucleus computes the seeds on the device and calls this.  Raises NucleusError as locate_nucleus
    does."""
    if not isinstance(view, WideDeepView):
        raise ValueError("locate_wide_nucleus takes a WideDeepView (a DeepView: locate_nucleus)")
    period, delta = seeds
    seed = pick_wide_nucleus_seed(view, period, delta)
    if seed is None:
        raise NucleusError("no seed", f"no pixel's Newton target lies in the view at mrd {mrd}")
    P = int(precision_bits) if precision_bits is not None else wide_nucleus_precision_bits(view)
    rounds = int(max_rounds) if max_rounds is not None else max(32, -(-P // 40))
    C0 = (_exact_fraction(orbit.center[0]), _exact_fraction(orbit.center[1]))
    n = refine_nucleus(C0[0] + seed.offset_r, C0[1] + seed.offset_i, seed.period, P, rounds)
    off = (_exact_fraction(n.center_r) - C0[0], _exact_fraction(n.center_i) - C0[1])
    unit = Fraction(2) ** view.exp2
    inside = abs(off[0]) * 2 <= Fraction(view.range_r) * unit and abs(off[1]) * 2 <= Fraction(view.range_i) * unit
    return replace(n, seed_pixel=seed.pixel, inside=bool(inside))


def interior_host(c, mrd: int) -> Tuple[int, int, int, float]:
    """mbk_interior_host: (count, period, cycle_len, de) of the pixel c = (c_r, c_i) on the host, without a device: the
    contract's four stages (include/mbk.h, "Interior views") compiled from the functions the kernel uses.  period 0 with
    count 0 is an unknown pixel: no cycle showed within mrd."""
    lib = L.load()
    n, p, cl, de = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    _check(lib, lib.mbk_interior_host(float(c[0]), float(c[1]), mrd, C.byref(n), C.byref(p), C.byref(cl), C.byref(de)))
    return int(n.value), int(p.value), int(cl.value), float(de.value)


def normal_value_host(zr: float, zi: float, dr: float, di: float, count: int) -> Tuple[float, float]:
    """mbk_normal_value_host: the unit normal (nx, ny) at one final state (include/mbk.h, "Relief shading") on the host, from
    the function the kernel uses; (0, 0) is the flat normal."""
    lib = L.load()
    out = (C.c_double * 2)()
    _check(lib, lib.mbk_normal_value_host(float(zr), float(zi), float(dr), float(di), int(count), out))
    return float(out[0]), float(out[1])


def relief_shade_host(nx: float, ny: float, lx: float, ly: float, h: float) -> int:
    """mbk_relief_shade_host: the brightness q in [0, 256] of a sample with normal (nx, ny) under the light (lx, ly) at
    height h."""
    return int(L.load().mbk_relief_shade_host(float(nx), float(ny), float(lx), float(ly), float(h)))


def stripe_state_host(c, mrd: int, *, density: int = 5, skip: int = 0) -> dict:
    """mbk_stripe_state_host: the exact stripe state of one pixel by coordinate on the host (include/mbk.h, "Stripe-average
    colouring"): {"n", "N", "S", "t_last", "mag", "cnt", "v"}."""
    lib = L.load()
    st = L.mbk_stripe_state()
    _check(lib, lib.mbk_stripe_state_host(float(c[0]), float(c[1]), int(mrd), int(density), int(skip), C.byref(st)))
    return {"n": int(st.n), "N": int(st.N), "S": float(st.S), "t_last": float(st.t_last), "mag": float(st.mag),
            "cnt": int(st.cnt), "v": float(st.v)}


def stripe_value_host(S: float, t_last: float, cnt: int, mag: float, count: int) -> float:
    """mbk_stripe_value_host: the value v of one exact state on the host, from the function the kernel uses."""
    return float(L.load().mbk_stripe_value_host(float(S), float(t_last), int(cnt), float(mag), int(count)))


def stripe_shade_host(v: float, lo: float, gain: float) -> int:
    """mbk_stripe_shade_host: the brightness q in [0, 256] of a sample with stripe average v."""
    return int(L.load().mbk_stripe_shade_host(float(v), float(lo), float(gain)))


def stripe_state_arrays(buf: np.ndarray, shape) -> dict:
    """The five arrays of a stripe state buffer (32 bytes per pixel: S, t_last, mag as float64, then N, cnt as int32), as
    views of ``buf`` (uint8, 32 * px bytes) shaped ``shape``."""
    px = int(shape[0]) * int(shape[1])
    f = buf[:24 * px].view(np.float64)
    i = buf[24 * px:32 * px].view(np.int32)
    return {"S": f[:px].reshape(shape), "t_last": f[px:2 * px].reshape(shape), "mag": f[2 * px:3 * px].reshape(shape),
            "N": i[:px].reshape(shape), "cnt": i[px:].reshape(shape)}


def _interior_spec(palette, supersample, unknown, outside, scale, max_band_rows):
    """(mbk_interior_render_spec, the palette array it points into) for a palette of uint8[n, 4] entries, entry k the colour
    of period k + 1."""
    pal = np.ascontiguousarray(getattr(palette, "entries", palette), dtype=np.uint8).reshape(-1, 4)
    spec = L.mbk_interior_render_spec(int(supersample), pal.ctypes.data if pal.size else None, pal.shape[0],
                                      (C.c_uint8 * 4)(*unknown), (C.c_uint8 * 4)(*outside), float(scale), int(max_band_rows))
    return spec, pal


def interior_resolve_host(counts, period, de, *, palette, supersample: int = 1, scale: float = 2.0 ** 80,
                          unknown=(0, 0, 0, 255), outside=(255, 255, 255, 255)) -> np.ndarray:
    """mbk_interior_resolve_host: the colour and resolve rules of an interior render on host samples of
    (height * s, width * s); returns uint8[height, width, 4]."""
    lib = L.load()
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    period = np.ascontiguousarray(period, dtype=np.int32)
    de = np.ascontiguousarray(de, dtype=np.float64)
    s = int(supersample)
    height, width = (counts.shape[0] // s, counts.shape[1] // s) if s > 0 else counts.shape
    spec, pal = _interior_spec(palette, s, unknown, outside, scale, 0)
    out = np.zeros((height, width, 4), np.uint8)
    _check(lib, lib.mbk_interior_resolve_host(C.byref(spec), width, height, counts.ctypes.data, period.ctypes.data, de.ctypes.data,
                                              out.ctypes.data if out.size else None))
    return out


def density_cell_host(target: DensityTarget, z) -> Optional[Tuple[int, int]]:
    """mbk_density_cell_host: the cell (x, y) of the point z = (z_r, z_i) in `target`, or None when it falls outside."""
    lib = L.load()
    ct = target.ctarget()
    cx, cy, inside = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    _check(lib, lib.mbk_density_cell_host(C.byref(ct), float(z[0]), float(z[1]), C.byref(cx), C.byref(cy), C.byref(inside)))
    return (int(cx.value), int(cy.value)) if inside.value else None


def density_host(view: View, target: DensityTarget, mrd: int, *, min_count: int = 1, max_count: int = 0, window=None,
                 out: Optional[np.ndarray] = None):
    """mbk_density_accumulate_host: the density table of a view / window on the host, one orbit at a time, without a device --
    the functions the kernels are compiled from.  ADDED into `out` (uint32[height, width]; None: zeros).
    Returns (table, DensityStats)."""
    lib = L.load()
    cv = MandelbrotDevice._cview(view, window)
    ct = target.ctarget()
    shape = (max(int(target.height), 0), max(int(target.width), 0))
    table = np.zeros(shape, np.uint32) if out is None else _out_array(out, shape, np.uint32)
    ds = L.mbk_density_stats()
    _check(lib, lib.mbk_density_accumulate_host(C.byref(cv), C.byref(ct), mrd, min_count, max_count,
                                                table.ctypes.data if table.size else None, C.byref(ds)))
    return table.reshape(shape), DensityStats(int(ds.deposits), int(ds.dropped))


def _stream_array(stream) -> np.ndarray:
    """A chunk stream (bytes, bytearray, memoryview or uint8 array) as a contiguous uint8 array, without a copy where possible."""
    if isinstance(stream, np.ndarray):
        a = np.ascontiguousarray(stream, dtype=np.uint8).ravel()
    else:
        a = np.frombuffer(stream, np.uint8)
    return a


_EMPTY_STREAM = (C.c_uint8 * 1)()   # what the pointer of an empty stream points to: never read, alive with the module


def _stream_ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else C.addressof(_EMPTY_STREAM)


class ChunkStreamError(MbkError):
    """An invalid chunk stream; `reason` is one of _lib.MBK_STREAM_* (include/mbk.h, "Stored chunks")."""

    def __init__(self, reason: int, message: str):
        super().__init__(L.MBK_ERR_INVALID, message)
        self.reason = reason


def chunk_stream_check(stream, n: int = L.MBK_CHUNK_BYTES) -> Tuple[int, int]:
    """mbk_chunk_stream_check on the host: (codec, runs) of a valid stream of an n-byte chunk; ChunkStreamError otherwise."""
    lib = L.load()
    a = _stream_array(stream)
    codec, runs, reason = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    st = lib.mbk_chunk_stream_check(_stream_ptr(a), a.size, n, C.byref(codec), C.byref(runs), C.byref(reason))
    if st != L.MBK_OK:
        raise ChunkStreamError(int(reason.value), _error_text(lib))
    return int(codec.value), int(runs.value)


def decode_chunk_host(stream, n: int = L.MBK_CHUNK_BYTES, out: Optional[np.ndarray] = None) -> np.ndarray:
    """mbk_chunk_decode_host: the decoded chunk (uint8[n]) without a device -- the functions the kernels are compiled from.
    `out` is left untouched when the stream is invalid (MbkError)."""
    lib = L.load()
    a = _stream_array(stream)
    out = _out_array(out, n, np.uint8)
    _check(lib, lib.mbk_chunk_decode_host(_stream_ptr(a), a.size, n, out.ctypes.data))
    return out


class MandelbrotDevice:
    """One mbk_ctx == one GPU.  Not thread-safe: use one host thread per instance."""

    SLOTS = L.MBK_SLOTS   # tiles in flight of the host-buffer API (submit_* / wait)
    WORKER_DEPTH = L.MBK_WORKER_DEPTH   # what the worker loops keep in flight (include/mbk.h)

    def __init__(self, device: int = 0):
        self._lib = L.load()
        h = C.c_void_p()
        _check(self._lib, self._lib.mbk_create(device, C.byref(h)))
        self._h = h
        self.device = device
        self._pinned = []
        self._ser_buf = np.empty(1 + L.MBK_CHUNK_BYTES, np.uint8)   # reused by serialize_last

    # -- lifecycle -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            for p in self._pinned:
                self._lib.mbk_host_free(self._h, p)
            self._pinned = []
            self._lib.mbk_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        _check(self._lib, st, self._h)

    # -- queries ---------------------------------------------------------------------------
    def info(self) -> dict:
        inf = L.mbk_device_info()
        self._check(self._lib.mbk_get_device_info(self._h, C.byref(inf)))
        return {"name": inf.name.decode(), "arch": inf.arch.decode(),
                "compute_units": inf.compute_units, "clock_mhz": inf.clock_mhz,
                "wavefront_size": inf.wavefront_size, "total_mem": inf.total_mem}

    def pci_bus_id(self) -> str:
        buf = C.create_string_buffer(32)
        self._check(self._lib.mbk_device_pci_bus_id(self._h, buf, 32))
        return buf.value.decode()

    def pinned_empty(self, shape, dtype) -> np.ndarray:
        """A numpy array over pinned host memory (freed when the device is closed)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._check(self._lib.mbk_host_alloc(self._h, max(n, 1), C.byref(p)))
        self._pinned.append(p)
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def set_option(self, name: str, value: int) -> None:
        """Tuning option (include/mbk.h enum mbk_option; names in _lib.OPTIONS).  Scheduling only:
        every accepted value gives bit-identical results."""
        self._check(self._lib.mbk_set_option(self._h, L.OPTIONS[name], int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_uint32(0)
        self._check(self._lib.mbk_get_option(self._h, L.OPTIONS[name], C.byref(v)))
        return int(v.value)

    def scan_occupancy(self) -> dict:
        """hipOccupancyMaxActiveBlocksPerMultiprocessor of the scan-path kernels (single-wave workgroups per CU)."""
        out = {}
        for k, name in enumerate(["f64_scan", "f64_heavy", "f32_scan", "f32_heavy"]):
            v = C.c_uint32(0)
            self._check(self._lib.mbk_get_option(self._h, L.MBK_INFO_SCAN_WG_PER_CU + k, C.byref(v)))
            out[name] = int(v.value)
        return out

    def xcd_shares(self) -> dict:
        """MBK_OPT_XCD_BALANCE = 1: the shares of the heavy list the eight XCDs currently get (an even deal is 0.125 each), the
        number of the last units launch whose time stamps were read, and the units launches issued."""
        vals = []
        for k in range(10):
            v = C.c_uint32(0)
            self._check(self._lib.mbk_get_option(self._h, L.MBK_INFO_XCD_SHARE + k, C.byref(v)))
            vals.append(int(v.value))
        return {"shares": [round(v / 1048576.0, 5) for v in vals[:8]], "last_launch_read": vals[8], "units_launches": vals[9]}

    def spill_info(self) -> dict:
        """SPILL (MBK_OPT_SPILL_FIRST): lanes the last launch with a second pass handed over to it, and how many launches of
        this context ran with one."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.mbk_get_option(self._h, L.MBK_INFO_SPILL, C.byref(a)))
        self._check(self._lib.mbk_get_option(self._h, L.MBK_INFO_SPILL + 1, C.byref(b)))
        return {"lanes_last_launch": int(a.value), "launches": int(b.value)}

    def quantise_counts(self, counts: np.ndarray, mrd: int) -> np.ndarray:
        """The device's quantiser alone (WorkerCUDA.py:96-98) on host int32 counts in [0, mrd-1]."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        out = np.empty(counts.shape, np.uint8)
        self._check(self._lib.mbk_quantise_counts(self._h, counts.ctypes.data, counts.size, mrd, out.ctypes.data))
        return out

    # -- compute ---------------------------------------------------------------------------
    @staticmethod
    def _cview(view: View, window) -> L.mbk_view:
        col0, row0, ncols, nrows = window if window is not None else (0, 0, view.width, view.height)
        return L.mbk_view(view.start_r, view.start_i, view.range_r, view.range_i,
                          view.width, view.height, col0, row0, ncols, nrows)

    def compute_view(self, view: View, mrd: int, *, window=None, want_counts: bool = True,
                     want_bytes: bool = True, kernel: str = "default", precision: str = "f64",
                     out_counts: Optional[np.ndarray] = None, out_bytes: Optional[np.ndarray] = None):
        """Synchronous: returns (counts int32[nrows,ncols] | None, bytes uint8[nrows,ncols] | None, TileStats)."""
        cv = self._cview(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = _out_array(out_counts, shape, np.int32) if want_counts else None
        byts = _out_array(out_bytes, shape, np.uint8) if want_bytes else None
        flags, p_counts, p_bytes = _wanted(shape, counts, byts)
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_compute(self._h, C.byref(cv), mrd, L.KERNELS[kernel] | L.PRECISIONS[precision] | flags,
                                               p_counts, p_bytes, C.byref(st)))
        return counts, byts, _stats(st)

    def datachunk(self, level: int, mrd: int, index_real: int, index_imag: int, *,
                  want_counts: bool = False, out_bytes: Optional[np.ndarray] = None):
        """The reference's process_workload (WorkerCUDA.py:70-100): uint8[16777216] for one tile.
        Returns (bytes uint8[16777216], counts int32[16777216] | None, TileStats)."""
        byts = _out_array(out_bytes, L.MBK_CHUNK_BYTES, np.uint8)
        counts = np.empty(L.MBK_CHUNK_BYTES, np.int32) if want_counts else None
        st = L.mbk_stats()
        self._check(self._lib.mbk_datachunk(
            self._h, level, mrd, index_real, index_imag, byts.ctypes.data,
            counts.ctypes.data if counts is not None else None, C.byref(st)))
        return byts, counts, _stats(st)

    def compute_view_smooth(self, view: View, mrd: int, *, window=None, kernel: str = "default"):
        """BASELINE cfg5 (not in the reference): continuous escape-time value nu = n + 1 - log2(0.5 ln|z_n|^2)
        at the reference's bailout, 0 for never-escaped pixels.
        Returns (smooth float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        cv = self._cview(view, window)
        shape = (cv.nrows, cv.ncols)
        smooth = np.empty(shape, np.float64)
        counts = np.empty(shape, np.int32)
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_compute_smooth(self._h, C.byref(cv), mrd, L.KERNELS[kernel],
                                                      counts.ctypes.data, smooth.ctypes.data, C.byref(st)))
        return smooth, counts, _stats(st)

    def launch_view_smooth(self, view: View, mrd: int, *, d_smooth: int, d_counts: int = 0, stream: int = 0,
                           window=None, kernel: str = "default") -> None:
        cv = self._cview(view, window)
        self._check(self._lib.mbk_view_launch_smooth(self._h, C.byref(cv), mrd, L.KERNELS[kernel],
                                                     d_counts or None, d_smooth, stream or None))

    def compute_view_distance(self, view: View, mrd: int, *, window=None, kernel: str = "default"):
        """Exterior distance estimates (not in the reference; include/mbk.h, "Distance estimates"): de = 2 |z| ln |z| / |dz/dc|
        in complex-plane units, evaluated after the orbit has run on to |z|^2 >= 2^32, 0 for never-escaped pixels.  The counts
        are those of compute_view.  kernel "asm" takes the one-pass form, every other selector computes the counts with that
        kernel first and the derivative in a second pass; both store the same values.
        Returns (distance float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        return self._distance_values("compute", "plain", view, mrd, window, kernel=kernel)

    def launch_view_distance(self, view: View, mrd: int, *, d_distance: int, d_counts: int = 0, stream: int = 0,
                             window=None, kernel: str = "default") -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 of the window's size) on ``stream`` (0 = HIP's null stream)."""
        self._distance_values("launch", "plain", view, mrd, window, d_values=d_distance, d_counts=d_counts, stream=stream, kernel=kernel)

    # -- interior views (include/mbk.h, "Interior views") -------------------------------------------
    def compute_view_interior(self, view: View, mrd: int, *, window=None, kernel: str = "default", want_counts: bool = True,
                              want_period: bool = True, want_distance: bool = True):
        """Periods and interior distance estimates (not in the reference): for every pixel that never escapes, the period of
        the attracting cycle its orbit settles on (0: none showed within mrd) and de = (1 - |A|^2) / |F + E B / (1 - A)| from the
        cycle's derivatives, in complex-plane units: true distance to the boundary <= de <= 4 x true distance.  Escaping pixels
        store 0 and 0.  The counts are those of compute_view.  kernel: "default", "scan" or "group", bit-identical.
        Returns (period int32[nrows,ncols] | None, distance float64[nrows,ncols] | None, counts int32[nrows,ncols] | None,
        TileStats)."""
        cv = self._cview(view, window)
        shape = (cv.nrows, cv.ncols)
        period = np.empty(shape, np.int32) if want_period else None
        dist = np.empty(shape, np.float64) if want_distance else None
        counts = np.empty(shape, np.int32) if want_counts else None
        st = L.mbk_stats()
        ptr = lambda a: a.ctypes.data if a is not None else None
        self._check(self._lib.mbk_view_interior_compute(self._h, C.byref(cv), mrd, L.KERNELS[kernel], ptr(counts), ptr(period),
                                                        ptr(dist), C.byref(st)))
        return period, dist, counts, _stats(st)

    def launch_view_interior(self, view: View, mrd: int, *, d_period: int = 0, d_distance: int = 0, d_counts: int = 0,
                             stream: int = 0, window=None, kernel: str = "default") -> None:
        """Asynchronous form on DEVICE pointers (int32 / float64 / int32 of the window's size; one of d_period, d_distance may
        be 0) on ``stream`` (0 = HIP's null stream)."""
        cv = self._cview(view, window)
        self._check(self._lib.mbk_view_interior_launch(self._h, C.byref(cv), mrd, L.KERNELS[kernel], d_counts or None,
                                                       d_period or None, d_distance or None, stream or None))

    def render_view_interior(self, view: View, mrd: int, *, palette, scale: float = 2.0 ** 80, supersample: int = 1,
                             unknown=(0, 0, 0, 255), outside=(255, 255, 255, 255), window=None, kernel: str = "default",
                             max_band_rows: int = 0, out: Optional[np.ndarray] = None):
        """The period map as an RGBA8 image: a sample of period p takes palette entry (p - 1) mod n (uint8[n, 4] or an
        image.Palette), its R, G, B scaled by min(de * scale, 1): scale = 2 ** 80 is the flat map, scale = 1 / (k * pitch)
        darkens the inner k pixels towards the boundary.  `outside` colours escaping samples, `unknown` those without a period.
        Supersampling, windows and bands as for render_view.  Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples)."""
        cv = self._cview(view, window)
        spec, pal = _interior_spec(palette, supersample, unknown, outside, scale, max_band_rows)
        img = self._render_out(cv, out)
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_interior_render_compute(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                               img.ctypes.data, C.byref(st)))
        return img, _stats(st)

    def launch_render_view_interior(self, view: View, mrd: int, *, palette, d_rgba: int, scale: float = 2.0 ** 80,
                                    supersample: int = 1, unknown=(0, 0, 0, 255), outside=(255, 255, 255, 255), stream: int = 0,
                                    window=None, kernel: str = "default", max_band_rows: int = 0) -> None:
        """Asynchronous interior render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream``."""
        cv = self._cview(view, window)
        spec, pal = _interior_spec(palette, supersample, unknown, outside, scale, max_band_rows)
        self._check(self._lib.mbk_view_interior_render_launch(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                              d_rgba or None, stream or None))

    # -- relief shading (include/mbk.h, "Relief shading") -------------------------------------------
    def compute_view_normals(self, view: View, mrd: int, *, window=None, kernel: str = "default", want_distance: bool = False):
        """Unit normals of the exterior potential (not in the reference): the direction of z / (dz/dc) at the final state of
        compute_view_distance, (0, 0) -- the flat normal -- for never-escaped pixels and where the state has overflowed.  The
        counts are those of compute_view.  kernel as for compute_view_distance; both forms store the same values.
        Returns (counts int32[nrows,ncols], normals float64[nrows,ncols,2], TileStats), with want_distance
        (counts, normals, distance float64[nrows,ncols], TileStats): the bits compute_view_distance stores."""
        cv = self._cview(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = np.empty(shape, np.int32)
        normals = np.empty(shape + (2,), np.float64)
        dist = np.empty(shape, np.float64) if want_distance else None
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_compute_normal(self._h, C.byref(cv), mrd, L.KERNELS[kernel], counts.ctypes.data,
                                                      normals.ctypes.data, dist.ctypes.data if want_distance else None, C.byref(st)))
        return (counts, normals, dist, _stats(st)) if want_distance else (counts, normals, _stats(st))

    def launch_view_normals(self, view: View, mrd: int, *, d_normals: int, d_counts: int = 0, d_distance: int = 0, stream: int = 0,
                            window=None, kernel: str = "default") -> None:
        """Asynchronous form on DEVICE pointers (float64 x 2 / int32 / float64 per pixel of the window; d_counts and d_distance
        may be 0) on ``stream`` (0 = HIP's null stream)."""
        cv = self._cview(view, window)
        self._check(self._lib.mbk_view_launch_normal(self._h, C.byref(cv), mrd, L.KERNELS[kernel], d_counts or None,
                                                     d_normals or None, d_distance or None, stream or None))

    def render_view_relief(self, view: View, mrd: int, *, palette, light_deg: float = 45.0, height: float = 1.5,
                           supersample: int = 1, window=None, max_band_rows: int = 0, kernel: str = "default", light=None,
                           out: Optional[np.ndarray] = None):
        """The view as a relief: the "smooth" colouring of render_view (image.Palette, its scale and offset) with R, G, B of
        every escaped sample scaled by how its normal faces a light from the direction light_deg (degrees, counter-clockwise
        from the positive real axis) at `height` above the plane -- filaments and spirals stand out as ridges.  height 0 is the
        harshest light, a large height flattens it.  light: the doubles (lx, ly) in place of (cos, sin) of light_deg.
        Supersampling, windows and bands as for render_view.  Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples)."""
        cv = self._cview(view, window)
        spec = palette.relief_spec(supersample, light_deg, height, max_band_rows, light=light)
        img = self._render_out(cv, out)
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_relief_render_compute(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                             img.ctypes.data, C.byref(st)))
        return img, _stats(st)

    def launch_render_view_relief(self, view: View, mrd: int, *, palette, d_rgba: int, light_deg: float = 45.0, height: float = 1.5,
                                  supersample: int = 1, stream: int = 0, window=None, max_band_rows: int = 0,
                                  kernel: str = "default", light=None) -> None:
        """Asynchronous relief render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream``."""
        cv = self._cview(view, window)
        spec = palette.relief_spec(supersample, light_deg, height, max_band_rows, light=light)
        self._check(self._lib.mbk_view_relief_render_launch(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                            d_rgba or None, stream or None))

    # -- stripe-average colouring (include/mbk.h, "Stripe-average colouring") -----------------------
    def compute_view_stripes(self, view: View, mrd: int, *, density: int = 5, skip: int = 0, window=None, kernel: str = "default",
                             want_state: bool = False):
        """Stripe averages (not in the reference): per pixel the mean of 1/2 + 1/2 sin(density arg z_k) over its own orbit,
        the first ``skip`` points left out, interpolated across the escape bands; 0 for never-escaped pixels.  The counts are
        those of compute_view.  kernel: "default", "scan" or "group".
        Returns (counts int32[nrows,ncols], v float64[nrows,ncols], TileStats), with want_state
        (counts, v, state, TileStats): state is the dict of stripe_state_arrays (S, t_last, mag, N, cnt)."""
        cv = self._cview(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = np.empty(shape, np.int32)
        v = np.empty(shape, np.float64)
        buf = np.empty(32 * cv.nrows * cv.ncols, np.uint8) if want_state else None
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_compute_stripe(self._h, C.byref(cv), mrd, L.KERNELS[kernel], int(density), int(skip),
                                                      counts.ctypes.data, v.ctypes.data, buf.ctypes.data if want_state else None,
                                                      C.byref(st)))
        return (counts, v, stripe_state_arrays(buf, shape), _stats(st)) if want_state else (counts, v, _stats(st))

    def launch_view_stripes(self, view: View, mrd: int, *, d_stripe: int, d_counts: int = 0, d_state: int = 0, density: int = 5,
                            skip: int = 0, stream: int = 0, window=None, kernel: str = "default") -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 / 32 bytes per pixel of the window; d_counts and d_state may
        be 0) on ``stream`` (0 = HIP's null stream).  d_state has the layout of stripe_state_arrays."""
        cv = self._cview(view, window)
        self._check(self._lib.mbk_view_launch_stripe(self._h, C.byref(cv), mrd, L.KERNELS[kernel], int(density), int(skip),
                                                     d_counts or None, d_stripe or None, d_state or None, stream or None))

    def render_view_stripes(self, view: View, mrd: int, *, palette, density: int = 5, skip: int = 0, lo: float = 0.35,
                            gain: float = 1.0, supersample: int = 1, window=None, max_band_rows: int = 0, kernel: str = "default",
                            out: Optional[np.ndarray] = None):
        """The view with stripes: the "smooth" colouring of render_view (image.Palette, its scale and offset) with R, G, B of
        every escaped sample scaled by its stripe average -- ``lo`` is the brightness of the darkest stripe, ``gain`` the
        contrast about the middle (0 gives one neutral brightness).  Supersampling, windows and bands as for render_view.
        Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples)."""
        cv = self._cview(view, window)
        spec = palette.stripe_spec(supersample, density, skip, lo, gain, max_band_rows)
        img = self._render_out(cv, out)
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_stripe_render_compute(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                             img.ctypes.data, C.byref(st)))
        return img, _stats(st)

    def launch_render_view_stripes(self, view: View, mrd: int, *, palette, d_rgba: int, density: int = 5, skip: int = 0,
                                   lo: float = 0.35, gain: float = 1.0, supersample: int = 1, stream: int = 0, window=None,
                                   max_band_rows: int = 0, kernel: str = "default") -> None:
        """Asynchronous stripe render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream``."""
        cv = self._cview(view, window)
        spec = palette.stripe_spec(supersample, density, skip, lo, gain, max_band_rows)
        self._check(self._lib.mbk_view_stripe_render_launch(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                            d_rgba or None, stream or None))

    def serialize_last(self) -> Tuple[bytes, int]:
        """The last tile's quantised bytes exactly as DataChunk.Serialize (DataChunk.cs:173-206) would
        write them (code byte + Raw or RLE payload, the shorter; Raw on ties), encoded on the GPU.
        Returns (stream, codec)."""
        cap = len(self._ser_buf)
        size, codec = C.c_uint64(0), C.c_uint32(0)
        st = self._lib.mbk_serialize_last(self._h, self._ser_buf.ctypes.data, cap, C.byref(size), C.byref(codec))
        if st == L.MBK_ERR_INVALID and size.value > cap:
            self._ser_buf = np.empty(size.value, np.uint8)
            st = self._lib.mbk_serialize_last(self._h, self._ser_buf.ctypes.data, size.value, C.byref(size),
                                              C.byref(codec))
        self._check(st)
        return self._ser_buf[:size.value].tobytes(), int(codec.value)

    def submit_datachunk(self, slot: int, level: int, mrd: int, index_real: int, index_imag: int,
                         out_bytes: np.ndarray, lazy_uniform: bool = False) -> None:
        """Enqueue a tile on `slot` (0 .. SLOTS-1) and return at once; `out_bytes` (uint8[16777216], ideally from
        pinned_empty) is valid after wait(slot).  Several slots = the D2H of one tile overlaps the kernels of the others.
        lazy_uniform (MBK_LAZY_UNIFORM): the caller does not need `out_bytes` when the tile turns out all-0 / all-1 -- the
        TileStats returned by wait() say which constant it is, and `out_bytes` is then unspecified: a tile wholly outside
        |c| = 2 costs no GPU work at all, the copy of a tile the host probe takes for all-exterior is decided when its
        statistics arrive, every other tile is copied as usual."""
        assert out_bytes.dtype == np.uint8 and out_bytes.size == L.MBK_CHUNK_BYTES and out_bytes.flags.c_contiguous
        self._check(self._lib.mbk_datachunk_submit_ex(self._h, slot, level, mrd, index_real, index_imag,
                                                      out_bytes.ctypes.data, None,
                                                      L.MBK_LAZY_UNIFORM if lazy_uniform else 0))

    def submit_view(self, slot: int, view: View, mrd: int, *, window=None, out_counts: Optional[np.ndarray] = None,
                    out_bytes: Optional[np.ndarray] = None, kernel: str = "default", precision: str = "f64") -> None:
        """Enqueue a view / window on `slot` and return at once; the given host arrays (C-contiguous, sized
        for the window; slices of a larger image are fine) are valid after wait(slot)."""
        cv = self._cview(view, window)
        flags, p_counts, p_bytes = _wanted((cv.nrows, cv.ncols), out_counts, out_bytes)
        self._check(self._lib.mbk_view_submit(self._h, slot, C.byref(cv), mrd, L.KERNELS[kernel] | L.PRECISIONS[precision] | flags,
                                              p_counts, p_bytes))

    def wait(self, slot: int) -> TileStats:
        st = L.mbk_stats()
        self._check(self._lib.mbk_wait(self._h, slot, C.byref(st)))
        return _stats(st)

    def launch_view(self, view: View, mrd: int, *, d_counts: int = 0, d_bytes: int = 0,
                    stream: int = 0, window=None, kernel: str = "default", precision: str = "f64") -> None:
        """Asynchronous launch on raw DEVICE pointers (e.g. torch tensors' data_ptr()) on ``stream``
        (a hipStream_t as int; 0 = HIP's null stream, which is also torch's default stream)."""
        cv = self._cview(view, window)
        flags = (L.KERNELS[kernel] | L.PRECISIONS[precision] | (L.MBK_WANT_COUNTS if d_counts else 0)
                 | (L.MBK_WANT_BYTES if d_bytes else 0))
        self._check(self._lib.mbk_view_launch(self._h, C.byref(cv), mrd, flags,
                                              d_counts or None, d_bytes or None, stream or None))

    # -- deep-zoom views (include/mbk.h, "Deep-zoom views") ------------------------------------
    # Every method below takes a DeepView or a WideDeepView ("Extended-range deep views"): the wide view goes to the
    # mbk_deep_xview_* call of the same name, which refuses the distance sources (the wide distance estimate has methods of
    # its own: compute_wide_view_distance, below) and has a bilinear approximation of its own (xbla, MBK_DEEP_XBLA; bla stays
    # refused there, and xbla is refused for a plain DeepView).
    @staticmethod
    def _cdeep(view: Union[DeepView, WideDeepView], window):
        col0, row0, ncols, nrows = window if window is not None else (0, 0, view.width, view.height)
        if isinstance(view, WideDeepView):
            return L.mbk_deep_xview(view.range_r, view.range_i, view.exp2, view.width, view.height, col0, row0, ncols, nrows)
        return L.mbk_deep_view(view.span_r, view.span_i, view.width, view.height, col0, row0, ncols, nrows)

    def _deep_fn(self, view, name: str, bla: bool = False, source: Optional[str] = None, xbla: bool = False):
        """(the C entry point `name` for this kind of deep view, its flags)"""
        if isinstance(view, WideDeepView):
            if bla:
                raise ValueError("bla=True is not implemented for a WideDeepView")
            if source in ("distance", "distance_rel"):
                raise ValueError("distance estimates are not implemented for a WideDeepView")
            return getattr(self._lib, "mbk_deep_xview_" + name), (L.MBK_DEEP_XBLA if xbla else 0)
        if xbla and bla:
            raise ValueError("bla=True and xbla=True exclude each other")
        if xbla:
            raise ValueError("xbla=True is implemented for a WideDeepView only (a DeepView takes bla=True)")
        return getattr(self._lib, "mbk_deep_view_" + name), (L.MBK_DEEP_BLA if bla else 0)

    # One body per operation serves the four kinds of view.  A kind is named by keywords: orbit (a deep view, plain or wide,
    # with bla), c (the Julia set of c on a view, with kernel), neither (a plain view, with kernel and precision).
    def _cany(self, view, window, orbit=None, **_):
        return self._cdeep(view, window) if orbit is not None else self._cview(view, window)

    def _kind_fn(self, name: str, view, cv, *, orbit=None, c=None, kernel: str = "default", precision: str = "f64", bla: bool = False,
                 source: Optional[str] = None, xbla: bool = False):
        """(the C entry point `name` for this kind of view, its arguments between the ctx and mrd, its flags)"""
        if orbit is not None:
            fn, flags = self._deep_fn(view, name, bla, source, xbla)
            return fn, (orbit._h, C.byref(cv)), flags
        if c is not None:
            return getattr(self._lib, "mbk_julia_view_" + name), (C.byref(cv), float(c[0]), float(c[1])), L.KERNELS[kernel]
        return getattr(self._lib, "mbk_view_" + name), (C.byref(cv),), L.KERNELS[kernel] | L.PRECISIONS[precision]

    # The distance rules (include/mbk.h, the "Distance estimates ..." sections): the C value calls of each, the renders of its own
    # and the one source they take (plain views and deep views without skips render through render_view / render_deep_view).
    _DISTANCE_RULES = {
        "plain": ("mbk_view_{}_distance", None, None),
        "julia": ("mbk_julia_view_{}_distance", "mbk_julia_view_distance_render_{}", "distance"),
        "deep": ("mbk_deep_view_{}_distance", None, None),
        "deep_bla": ("mbk_deep_view_{}_distance_bla", "mbk_deep_view_distance_bla_render_{}", "distance_rel"),
        "wide": ("mbk_deep_xview_{}_distance", "mbk_deep_xview_distance_render_{}", "distance_rel"),
        "wide_xbla": ("mbk_deep_xview_{}_distance_xbla", "mbk_deep_xview_distance_xbla_render_{}", "distance_rel"),
    }

    def _distance_args(self, rule: str, view, window, *, orbit=None, c=None, kernel: str = "default"):
        """(the C view of the rule's kind, the arguments between the ctx and mrd, the flags): as _kind_fn names a kind, and only
        the rules without an orbit select a kernel."""
        if orbit is not None:
            cv = _cxview(view, window) if rule.startswith("wide") else self._cdeep(view, window)
            return cv, (orbit._h, C.byref(cv)), 0
        cv = self._cview(view, window)
        return cv, (C.byref(cv),) + ((float(c[0]), float(c[1])) if c is not None else ()), L.KERNELS[kernel]

    def _distance_values(self, form: str, rule: str, view, mrd: int, window, *, d_values: int = 0, d_counts: int = 0, stream: int = 0,
                         **kind):
        """compute_*_distance* (form "compute": returns (values float64[nrows,ncols], counts int32[nrows,ncols], TileStats)) and
        launch_*_distance* (form "launch": into d_values and, where given, d_counts on `stream`) of any rule."""
        cv, lead, flags = self._distance_args(rule, view, window, **kind)
        fn = getattr(self._lib, self._DISTANCE_RULES[rule][0].format(form))
        if form == "launch":
            self._check(fn(self._h, *lead, mrd, flags, d_counts or None, d_values or None, stream or None))
            return None
        shape = (cv.nrows, cv.ncols)
        values = np.empty(shape, np.float64)
        counts = np.empty(shape, np.int32)
        st = L.mbk_stats()
        self._check(fn(self._h, *lead, mrd, flags, counts.ctypes.data, values.ctypes.data, C.byref(st)))
        return values, counts, _stats(st)

    def _distance_render(self, form: str, rule: str, view, mrd: int, palette, supersample, window, max_band_rows, *, out=None,
                         d_rgba: int = 0, stream: int = 0, **kind):
        """render_*_distance* (form "compute": into the host array `out`, returns (rgba, TileStats)) and launch_render_*_distance*
        (form "launch": into d_rgba on `stream`) of the rules that have renders of their own."""
        cv, lead, flags = self._distance_args(rule, view, window, **kind)
        _, name, source = self._DISTANCE_RULES[rule]
        rgba = self._render_out(cv, out) if form == "compute" else None
        spec = palette.spec(source, supersample, max_band_rows)
        st = L.mbk_stats()
        tail = (rgba.ctypes.data, C.byref(st)) if form == "compute" else (d_rgba or None, stream or None)
        self._check(getattr(self._lib, name.format(form))(self._h, *lead, mrd, flags, C.byref(spec), *tail))
        return (rgba, _stats(st)) if form == "compute" else None

    def _render(self, form: str, view, mrd: int, palette, source, supersample, window, max_band_rows, lut, histogram, *, out=None,
                d_rgba: int = 0, stream: int = 0, **kind):
        """render_* (form "compute": into the host array `out`, returns (rgba, TileStats)) and launch_render_* (form "launch":
        into d_rgba on `stream`) of any kind of view; histogram() is the whole view's, for source "equalized" without a lut."""
        cv = self._cany(view, window, **kind)
        rgba = self._render_out(cv, out) if form == "compute" else None
        spec = palette.spec(source, supersample, max_band_rows)
        equalized = source == "equalized"
        fn, lead, flags = self._kind_fn(("render_equalized_" if equalized else "render_") + form, view, cv, source=source, **kind)
        table = ()
        if equalized:
            lut = self._lut(lut, histogram)
            table = (lut.ctypes.data, lut.size)
        st = L.mbk_stats()
        tail = (rgba.ctypes.data, C.byref(st)) if form == "compute" else (d_rgba or None, stream or None)
        self._check(fn(self._h, *lead, mrd, flags, C.byref(spec), *table, *tail))
        return (rgba, _stats(st)) if form == "compute" else None

    def _histogram(self, view, mrd: int, window, want_stats: bool, **kind):
        cv = self._cany(view, window, **kind)
        hist = np.empty(max(int(mrd), 0), np.uint64)
        st = L.mbk_stats()
        fn, lead, flags = self._kind_fn("histogram_compute", view, cv, **kind)
        self._check(fn(self._h, *lead, mrd, flags, hist.ctypes.data if hist.size else None, C.byref(st)))
        return (hist, _stats(st)) if want_stats else hist

    def _launch_histogram(self, view, mrd: int, d_hist: int, stream: int, window, **kind) -> None:
        cv = self._cany(view, window, **kind)
        fn, lead, flags = self._kind_fn("histogram_launch", view, cv, **kind)
        self._check(fn(self._h, *lead, mrd, flags, d_hist or None, stream or None))

    def compute_deep_view(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None, want_counts: bool = True,
                          want_bytes: bool = True, want_smooth: bool = False, out_counts: Optional[np.ndarray] = None,
                          out_bytes: Optional[np.ndarray] = None, bla: bool = False, xbla: bool = False):
        """Synchronous: (counts int32 | None, bytes uint8 | None, smooth float64 | None, TileStats), each [nrows, ncols].
        bla: step with bilinear approximation (MBK_DEEP_BLA; include/mbk.h, "Deep-zoom views with bilinear approximation"):
        runs of steps collapse into one linear map while the pixel's offset is tiny against the reference orbit -- several
        times fewer steps on a deep view, counts that equal the exact rule's on all but a fraction of a percent of pixels.
        xbla: the same for a WideDeepView (MBK_DEEP_XBLA; "Extended-range deep views with bilinear approximation"): a table
        of its own, mantissas with int32 exponents.  bla with a WideDeepView and xbla with a DeepView are refused."""
        cv = self._cdeep(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = _out_array(out_counts, shape, np.int32) if want_counts else None
        byts = _out_array(out_bytes, shape, np.uint8) if want_bytes else None
        smooth = np.empty(shape, np.float64) if want_smooth else None
        flags, p_counts, p_bytes = _wanted(shape, counts, byts)
        fn, extra = self._deep_fn(view, "compute", bla, xbla=xbla)
        st = L.mbk_stats()
        self._check(fn(self._h, orbit._h, C.byref(cv), mrd, flags | extra, p_counts, p_bytes,
                       smooth.ctypes.data if smooth is not None else None, C.byref(st)))
        return counts, byts, smooth, _stats(st)

    def submit_deep_view(self, slot: int, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None,
                         out_counts: Optional[np.ndarray] = None, out_bytes: Optional[np.ndarray] = None,
                         bla: bool = False, xbla: bool = False) -> None:
        """Enqueue a deep view / window on `slot`; the host arrays are valid after wait(slot)."""
        cv = self._cdeep(view, window)
        flags, p_counts, p_bytes = _wanted((cv.nrows, cv.ncols), out_counts, out_bytes)
        fn, extra = self._deep_fn(view, "submit", bla, xbla=xbla)
        self._check(fn(self._h, slot, orbit._h, C.byref(cv), mrd, flags | extra, p_counts, p_bytes))

    def launch_deep_view(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, d_counts: int = 0, d_bytes: int = 0,
                         d_smooth: int = 0, stream: int = 0, window=None, bla: bool = False, xbla: bool = False) -> None:
        """Asynchronous launch on raw DEVICE pointers on ``stream`` (0 = HIP's null stream).  With bla or xbla the first launch of a
        view's spans on an orbit builds and uploads the table synchronously."""
        cv = self._cdeep(view, window)
        fn, extra = self._deep_fn(view, "launch", bla, xbla=xbla)
        flags = (L.MBK_WANT_COUNTS if d_counts else 0) | (L.MBK_WANT_BYTES if d_bytes else 0) | extra
        self._check(fn(self._h, orbit._h, C.byref(cv), mrd, flags, d_counts or None, d_bytes or None, d_smooth or None,
                       stream or None))

    def compute_deep_view_distance(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None):
        """Exterior distance estimates of a deep view (include/mbk.h, "Distance estimates for deep views"): the derivative is
        carried as D 2^e, so it cannot overflow however deep the view, and the value is rel = de / span_r, the distance as a
        fraction of the view's real span (rel * (width - 1) is the distance in pixels); 0 for never-escaped pixels.  The counts
        are those of compute_deep_view.  Returns (rel float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        self._deep_fn(view, "compute_distance", source="distance_rel")   # (a WideDeepView: compute_wide_view_distance)
        return self._distance_values("compute", "deep", view, mrd, window, orbit=orbit)

    def launch_deep_view_distance(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, d_rel: int, d_counts: int = 0,
                                  stream: int = 0, window=None) -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 of the window's size) on ``stream`` (0 = HIP's null stream)."""
        self._deep_fn(view, "launch_distance", source="distance_rel")
        self._distance_values("launch", "deep", view, mrd, window, d_values=d_rel, d_counts=d_counts, stream=stream, orbit=orbit)

    # -- locating minibrots (include/mbk.h, "Locating minibrots in deep views") --
    @staticmethod
    def _nucleus_view(view) -> None:
        if not isinstance(view, DeepView):
            raise ValueError("the deep_view_nucleus calls take a DeepView (a WideDeepView: the wide_view_nucleus calls)")

    def compute_deep_view_nucleus(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None):
        """Atom periods and Newton seeds of a deep view: per pixel the period p = 1 + the step at which |z| was smallest, and
        delta, one Newton step from the pixel towards the root of z_p(c) = 0 as a fraction of span_r (+inf in both components:
        no seed); the pixel's own offset is not included.  The counts are those of compute_deep_view.
        Returns (period int32[nrows,ncols], delta float64[nrows,ncols,2], counts int32[nrows,ncols], TileStats)."""
        self._nucleus_view(view)
        cv = self._cdeep(view, window)
        shape = (cv.nrows, cv.ncols)
        period = np.empty(shape, np.int32)
        delta = np.empty(shape + (2,), np.float64)
        counts = np.empty(shape, np.int32)
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_view_compute_nucleus(self._h, orbit._h, C.byref(cv), mrd, 0, counts.ctypes.data,
                                                            period.ctypes.data, delta.ctypes.data, C.byref(st)))
        return period, delta, counts, _stats(st)

    def launch_deep_view_nucleus(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, d_period: int, d_delta: int,
                                 d_counts: int = 0, stream: int = 0, window=None) -> None:
        """Asynchronous form on DEVICE pointers (int32, 2 x float64 and int32 per pixel of the window) on ``stream`` (0 = HIP's
        null stream)."""
        self._nucleus_view(view)
        cv = self._cdeep(view, window)
        self._check(self._lib.mbk_deep_view_launch_nucleus(self._h, orbit._h, C.byref(cv), mrd, 0, d_counts or None,
                                                           d_period or None, d_delta or None, stream or None))

    def locate_nucleus(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, precision_bits: Optional[int] = None, seeds=None,
                       max_rounds: int = 32) -> Nucleus:
        """Find the minibrot in this view: atom periods and Newton seeds on the device (or `seeds` = (period, delta)), the seed
        pick_nucleus_seed chooses, refine_nucleus on the host.  Nucleus.orbit(mrd) and Nucleus.view(width, height) then show it."""
        self._nucleus_view(view)
        if seeds is None:
            period, delta, _, _ = self.compute_deep_view_nucleus(orbit, view, mrd)
            seeds = (period, delta)
        return locate_nucleus(orbit, view, mrd, seeds=seeds, precision_bits=precision_bits, max_rounds=max_rounds)

    # -- the same from extended-range views (include/mbk.h, "Locating minibrots in extended-range deep views"): calls of their
    # own; the plain calls above keep refusing a WideDeepView --
    @staticmethod
    def _wide_nucleus_view(view) -> None:
        if not isinstance(view, WideDeepView):
            raise ValueError("the wide_view_nucleus calls take a WideDeepView (a DeepView: the deep_view_nucleus calls)")

    def compute_wide_view_nucleus(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, window=None):
        """compute_deep_view_nucleus for a WideDeepView: the candidates are ordered by a wide |z|^2 (near a deep minibrot |z| is
        1e-400: its square is 0 in binary64), the kept state is wide, and delta is the Newton step as a fraction of the view's
        real span range_r 2^exp2 (+inf in both components: no seed); the pixel's own offset is not included.  The counts are
        those of compute_deep_view.
        Returns (period int32[nrows,ncols], delta float64[nrows,ncols,2], counts int32[nrows,ncols], TileStats)."""
        self._wide_nucleus_view(view)
        cv = _cxview(view, window)
        shape = (cv.nrows, cv.ncols)
        period = np.empty(shape, np.int32)
        delta = np.empty(shape + (2,), np.float64)
        counts = np.empty(shape, np.int32)
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_xview_compute_nucleus(self._h, orbit._h, C.byref(cv), mrd, 0, counts.ctypes.data,
                                                             period.ctypes.data, delta.ctypes.data, C.byref(st)))
        return period, delta, counts, _stats(st)

    def launch_wide_view_nucleus(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, d_period: int, d_delta: int,
                                 d_counts: int = 0, stream: int = 0, window=None) -> None:
        """Asynchronous form on DEVICE pointers (int32, 2 x float64 and int32 per pixel of the window) on ``stream`` (0 = HIP's
        null stream)."""
        self._wide_nucleus_view(view)
        cv = _cxview(view, window)
        self._check(self._lib.mbk_deep_xview_launch_nucleus(self._h, orbit._h, C.byref(cv), mrd, 0, d_counts or None,
                                                            d_period or None, d_delta or None, stream or None))

    def locate_wide_nucleus(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, precision_bits: Optional[int] = None,
                            seeds=None, max_rounds: Optional[int] = None) -> Nucleus:
        """locate_nucleus from a WideDeepView: atom periods and Newton seeds on the device (or `seeds` = (period, delta)), the
        seed pick_wide_nucleus_seed chooses, refine_nucleus on the host.  With Nucleus.view and Nucleus.orbit the chain view ->
        nucleus -> view goes on below 2^-960."""
        self._wide_nucleus_view(view)
        if seeds is None:
            period, delta, _, _ = self.compute_wide_view_nucleus(orbit, view, mrd)
            seeds = (period, delta)
        return locate_wide_nucleus(orbit, view, mrd, seeds=seeds, precision_bits=precision_bits, max_rounds=max_rounds)

    # -- distance estimates for deep views with bilinear approximation (include/mbk.h, the section of that name): calls of
    # their own; compute_deep_view_distance and render_deep_view(source="distance_rel") keep refusing bla --
    @staticmethod
    def _plain_deep(view) -> None:
        if not isinstance(view, DeepView):
            raise ValueError("distance estimates with bilinear approximation are implemented for a DeepView only")

    def compute_deep_view_distance_bla(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None):
        """compute_deep_view_distance with the skips of compute_deep_view(bla=True): across a skip dz -> A dz + B dc the derivative
        follows d -> A d + B, from the table the count launches use.  The counts are those of compute_deep_view(bla=True); rel
        is within 1e-4 of the truth on the project's cases (tests/deep_distance_bla_model.py has the measured figures).
        Returns (rel float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        self._plain_deep(view)
        return self._distance_values("compute", "deep_bla", view, mrd, window, orbit=orbit)

    def launch_deep_view_distance_bla(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, d_rel: int, d_counts: int = 0,
                                      stream: int = 0, window=None) -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 of the window's size) on ``stream`` (0 = HIP's null stream).  The
        first launch of a view's spans on an orbit builds and uploads the table synchronously."""
        self._plain_deep(view)
        self._distance_values("launch", "deep_bla", view, mrd, window, d_values=d_rel, d_counts=d_counts, stream=stream, orbit=orbit)

    def render_deep_view_distance_bla(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, supersample: int = 1,
                                      window=None, max_band_rows: int = 0, out: Optional[np.ndarray] = None):
        """The view as an RGBA8 image coloured by that estimate (source "distance_rel"; Palette.deep_distance), as
        render_deep_view(source="distance_rel") does without skips.  Returns (rgba uint8[nrows, ncols, 4], TileStats)."""
        self._plain_deep(view)
        return self._distance_render("compute", "deep_bla", view, mrd, palette, supersample, window, max_band_rows, out=out, orbit=orbit)

    def launch_render_deep_view_distance_bla(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, d_rgba: int,
                                             supersample: int = 1, stream: int = 0, window=None, max_band_rows: int = 0) -> None:
        """Asynchronous render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream`` (0 = HIP's null stream)."""
        self._plain_deep(view)
        self._distance_render("launch", "deep_bla", view, mrd, palette, supersample, window, max_band_rows, d_rgba=d_rgba, stream=stream,
                              orbit=orbit)

    # -- relief shading for deep views (include/mbk.h, "Relief shading for deep views"): one pass per sample, whatever is asked --
    def compute_deep_view_normals(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None, bla: bool = False,
                                  want_smooth: bool = False, want_distance: bool = False):
        """Unit normals of the exterior potential of a deep view: compute_view_normals from the state compute_deep_view_distance
        (bla: compute_deep_view_distance_bla) ends with -- the scale 2^e of the derivative drops out of the direction.  (0, 0)
        for never-escaped pixels.  The counts are those of compute_deep_view(bla=bla); want_smooth adds its smooth values,
        want_distance the rel of the distance call, each bit for bit, from the same single pass.
        Returns (counts int32[nrows,ncols], normals float64[nrows,ncols,2], [smooth float64[nrows,ncols],]
        [rel float64[nrows,ncols],] TileStats)."""
        _no_wide_relief(view)
        cv = self._cdeep(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = np.empty(shape, np.int32)
        normals = np.empty(shape + (2,), np.float64)
        smooth = np.empty(shape, np.float64) if want_smooth else None
        rel = np.empty(shape, np.float64) if want_distance else None
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_view_compute_normal(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_BLA if bla else 0,
                                                           counts.ctypes.data, normals.ctypes.data,
                                                           smooth.ctypes.data if want_smooth else None,
                                                           rel.ctypes.data if want_distance else None, C.byref(st)))
        return (counts, normals) + ((smooth,) if want_smooth else ()) + ((rel,) if want_distance else ()) + (_stats(st),)

    def launch_deep_view_normals(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, d_normals: int, d_counts: int = 0,
                                 d_smooth: int = 0, d_rel: int = 0, stream: int = 0, window=None, bla: bool = False) -> None:
        """Asynchronous form on DEVICE pointers (float64 x 2 / int32 / float64 / float64 per pixel of the window; d_counts,
        d_smooth and d_rel may be 0) on ``stream`` (0 = HIP's null stream).  With bla the first launch of a view's spans on an
        orbit builds and uploads the table synchronously."""
        _no_wide_relief(view)
        cv = self._cdeep(view, window)
        self._check(self._lib.mbk_deep_view_launch_normal(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_BLA if bla else 0,
                                                          d_counts or None, d_normals or None, d_smooth or None, d_rel or None,
                                                          stream or None))

    def render_deep_view_relief(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, light_deg: float = 45.0,
                                height: float = 1.5, light=None, supersample: int = 1, window=None, max_band_rows: int = 0,
                                bla: bool = False, out: Optional[np.ndarray] = None):
        """The deep view as a relief: render_view_relief's light on render_deep_view's "smooth" colouring, every sample computed
        once.  Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples)."""
        _no_wide_relief(view)
        cv = self._cdeep(view, window)
        spec = palette.relief_spec(supersample, light_deg, height, max_band_rows, light=light)
        img = self._render_out(cv, out)
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_view_relief_render_compute(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_BLA if bla else 0,
                                                                  C.byref(spec), img.ctypes.data, C.byref(st)))
        return img, _stats(st)

    def launch_render_deep_view_relief(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, d_rgba: int,
                                       light_deg: float = 45.0, height: float = 1.5, light=None, supersample: int = 1,
                                       stream: int = 0, window=None, max_band_rows: int = 0, bla: bool = False) -> None:
        """Asynchronous relief render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream``."""
        _no_wide_relief(view)
        cv = self._cdeep(view, window)
        spec = palette.relief_spec(supersample, light_deg, height, max_band_rows, light=light)
        self._check(self._lib.mbk_deep_view_relief_render_launch(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_BLA if bla else 0,
                                                                 C.byref(spec), d_rgba or None, stream or None))

    # -- relief shading for extended-range deep views (include/mbk.h, the section of that name): calls of their own, one pass
    # per sample; the compute_deep_view_normals family keeps refusing a WideDeepView --
    def compute_wide_view_normals(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, window=None, xbla: bool = False,
                                  want_smooth: bool = False, want_distance: bool = False):
        """compute_deep_view_normals for a WideDeepView: unit normals of the exterior potential from the state
        compute_wide_view_distance (xbla: compute_wide_view_distance_xbla) ends with -- neither the exponent of z nor that of
        the derivative enters the direction.  (0, 0) for never-escaped pixels, and for no escaped one.  The counts are those of
        compute_deep_view(xbla=xbla); want_smooth adds its smooth values, want_distance the rel of the distance call, each bit
        for bit, from the same single pass.
        Returns (counts int32[nrows,ncols], normals float64[nrows,ncols,2], [smooth float64[nrows,ncols],]
        [rel float64[nrows,ncols],] TileStats)."""
        _wide_relief_only(view, "compute_wide_view_normals", "compute_deep_view_normals")
        cv = _cxview(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = np.empty(shape, np.int32)
        normals = np.empty(shape + (2,), np.float64)
        smooth = np.empty(shape, np.float64) if want_smooth else None
        rel = np.empty(shape, np.float64) if want_distance else None
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_xview_compute_normal(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_XBLA if xbla else 0,
                                                            counts.ctypes.data, normals.ctypes.data,
                                                            smooth.ctypes.data if want_smooth else None,
                                                            rel.ctypes.data if want_distance else None, C.byref(st)))
        return (counts, normals) + ((smooth,) if want_smooth else ()) + ((rel,) if want_distance else ()) + (_stats(st),)

    def launch_wide_view_normals(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, d_normals: int, d_counts: int = 0,
                                 d_smooth: int = 0, d_rel: int = 0, stream: int = 0, window=None, xbla: bool = False) -> None:
        """Asynchronous form on DEVICE pointers (float64 x 2 / int32 / float64 / float64 per pixel of the window; d_counts,
        d_smooth and d_rel may be 0) on ``stream`` (0 = HIP's null stream).  With xbla the first launch of a view's spans on an
        orbit builds and uploads the table synchronously."""
        _wide_relief_only(view, "launch_wide_view_normals", "launch_deep_view_normals")
        cv = _cxview(view, window)
        self._check(self._lib.mbk_deep_xview_launch_normal(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_XBLA if xbla else 0,
                                                           d_counts or None, d_normals or None, d_smooth or None, d_rel or None,
                                                           stream or None))

    def render_wide_view_relief(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, light_deg: float = 45.0,
                                height: float = 1.5, light=None, supersample: int = 1, window=None, max_band_rows: int = 0,
                                xbla: bool = False, out: Optional[np.ndarray] = None):
        """The extended-range view as a relief: render_view_relief's light on render_deep_view's "smooth" colouring, every
        sample computed once.  xbla: the samples are those of the s-times view under compute_deep_view(xbla=True), with that
        view's own table.  Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples)."""
        _wide_relief_only(view, "render_wide_view_relief", "render_deep_view_relief")
        cv = _cxview(view, window)
        spec = palette.relief_spec(supersample, light_deg, height, max_band_rows, light=light)
        img = self._render_out(cv, out)
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_xview_relief_render_compute(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_XBLA if xbla else 0,
                                                                   C.byref(spec), img.ctypes.data, C.byref(st)))
        return img, _stats(st)

    def launch_render_wide_view_relief(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, d_rgba: int,
                                       light_deg: float = 45.0, height: float = 1.5, light=None, supersample: int = 1,
                                       stream: int = 0, window=None, max_band_rows: int = 0, xbla: bool = False) -> None:
        """Asynchronous relief render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream``."""
        _wide_relief_only(view, "launch_render_wide_view_relief", "launch_render_deep_view_relief")
        cv = _cxview(view, window)
        spec = palette.relief_spec(supersample, light_deg, height, max_band_rows, light=light)
        self._check(self._lib.mbk_deep_xview_relief_render_launch(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_XBLA if xbla else 0,
                                                                  C.byref(spec), d_rgba or None, stream or None))

    # -- distance estimates for extended-range deep views (include/mbk.h, the section of that name): calls of their own --
    def compute_wide_view_distance(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, window=None):
        """compute_deep_view_distance for a WideDeepView: the derivative lives in the wide number system (binary64 mantissas,
        an int32 exponent), so neither a span of 2^-3000 nor an orbit that returns to within 1e-400 of 0 loses it.  The value
        is rel = de / (range_r 2^exp2), the distance as a fraction of the view's real span; the counts are those of
        compute_deep_view.  Returns (rel float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        return self._distance_values("compute", "wide", view, mrd, window, orbit=orbit)

    def launch_wide_view_distance(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, d_rel: int, d_counts: int = 0,
                                  stream: int = 0, window=None) -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 of the window's size) on ``stream`` (0 = HIP's null stream)."""
        self._distance_values("launch", "wide", view, mrd, window, d_values=d_rel, d_counts=d_counts, stream=stream, orbit=orbit)

    def render_wide_view_distance(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, supersample: int = 1,
                                  window=None, max_band_rows: int = 0, out: Optional[np.ndarray] = None):
        """The view as an RGBA8 image coloured by its distance estimate (source "distance_rel"; Palette.deep_distance), as
        render_deep_view(source="distance_rel") does for a DeepView.  Returns (rgba uint8[nrows, ncols, 4], TileStats)."""
        return self._distance_render("compute", "wide", view, mrd, palette, supersample, window, max_band_rows, out=out, orbit=orbit)

    def launch_render_wide_view_distance(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, d_rgba: int,
                                         supersample: int = 1, stream: int = 0, window=None, max_band_rows: int = 0) -> None:
        """Asynchronous render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream`` (0 = HIP's null stream)."""
        self._distance_render("launch", "wide", view, mrd, palette, supersample, window, max_band_rows, d_rgba=d_rgba, stream=stream,
                              orbit=orbit)

    # -- distance estimates for extended-range deep views with bilinear approximation (include/mbk.h, the section of that
    # name): calls of their own; compute_wide_view_distance keeps its rule and the flag stays refused there --
    def compute_wide_view_distance_xbla(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, window=None):
        """compute_wide_view_distance with the skips of compute_deep_view(xbla=True): across a skip dz -> A dz + B dc the
        derivative follows d -> A d + B, from the table the count launches use.  The counts are those of
        compute_deep_view(xbla=True); tests/deep_wide_distance_bla_model.py has the measured error of rel.
        Returns (rel float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        return self._distance_values("compute", "wide_xbla", view, mrd, window, orbit=orbit)

    def launch_wide_view_distance_xbla(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, d_rel: int, d_counts: int = 0,
                                       stream: int = 0, window=None) -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 of the window's size) on ``stream`` (0 = HIP's null stream).  The
        first launch of a view's spans on an orbit builds and uploads the table synchronously."""
        self._distance_values("launch", "wide_xbla", view, mrd, window, d_values=d_rel, d_counts=d_counts, stream=stream, orbit=orbit)

    def render_wide_view_distance_xbla(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, supersample: int = 1,
                                       window=None, max_band_rows: int = 0, out: Optional[np.ndarray] = None):
        """The view as an RGBA8 image coloured by that estimate (source "distance_rel"; Palette.deep_distance), as
        render_wide_view_distance does without skips.  Returns (rgba uint8[nrows, ncols, 4], TileStats)."""
        return self._distance_render("compute", "wide_xbla", view, mrd, palette, supersample, window, max_band_rows, out=out, orbit=orbit)

    def launch_render_wide_view_distance_xbla(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, d_rgba: int,
                                              supersample: int = 1, stream: int = 0, window=None, max_band_rows: int = 0) -> None:
        """Asynchronous render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream`` (0 = HIP's null stream)."""
        self._distance_render("launch", "wide_xbla", view, mrd, palette, supersample, window, max_band_rows, d_rgba=d_rgba, stream=stream,
                              orbit=orbit)

    # -- rendering (include/mbk.h, "Rendering") ---------------------------------------------------
    def _render_out(self, cv, out):
        shape = (cv.nrows, cv.ncols, 4)
        return _out_array(out, shape, np.uint8).reshape(shape)

    def render_view(self, view: View, mrd: int, *, palette, source: str = "smooth", supersample: int = 1, window=None,
                    kernel: str = "default", max_band_rows: int = 0, out: Optional[np.ndarray] = None, lut=None):
        """The view as an RGBA8 image, coloured and anti-aliased on the GPU: (width * s) x (height * s) samples of the
        same rectangle, each through `palette` (image.Palette; source "smooth": nu, "bytes": the quantised byte,
        "distance": the exterior distance estimate, palette not cyclic -- Palette.distance), s x s of them averaged per pixel.  Only the image crosses PCIe.  `window` is in output pixels; `out` may be a
        (pinned) uint8 array of the window's size.  Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples);
        row 0 is the lowest imaginary part.
        Source "equalized" colours nu through an equalisation table (image.equalize_lut; Palette.for_equalized): `lut`, or
        with lut=None the table of the histogram of the WHOLE view at output resolution (view_histogram: s = 1, `window`
        ignored, so that every band of an image, on any GPU, uses one table); 8 * mrd bytes and the image cross PCIe."""
        return self._render("compute", view, mrd, palette, source, supersample, window, max_band_rows, lut,
                            lambda: self.view_histogram(view, mrd, kernel=kernel), out=out, kernel=kernel)

    @staticmethod
    def _lut(lut, histogram) -> np.ndarray:
        """The caller's equalisation table as a contiguous float64 array, or the table of histogram()."""
        if lut is None:
            from .image import equalize_lut
            return equalize_lut(histogram())
        return np.ascontiguousarray(lut, dtype=np.float64).ravel()

    def render_deep_view(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, source: str = "smooth",
                         supersample: int = 1, window=None, max_band_rows: int = 0, out: Optional[np.ndarray] = None, lut=None,
                         bla: bool = False, xbla: bool = False):
        """render_view for a deep view: the samples are those of the same orbit and spans at s times the width and height.
        Source "distance_rel" colours the deep distance estimate (compute_deep_view_distance; Palette.deep_distance); source
        "distance", the plain views' estimate in plane units, is refused (MbkError).  Source "equalized" and `lut` as for
        render_view (the table of deep_view_histogram of the whole view when lut is None).  bla: the samples (and that
        histogram) are those of compute_deep_view(bla=True); refused with source "distance_rel".  xbla: likewise for a
        WideDeepView (compute_deep_view(xbla=True))."""
        return self._render("compute", view, mrd, palette, source, supersample, window, max_band_rows, lut,
                            lambda: self.deep_view_histogram(orbit, view, mrd, bla=bla, xbla=xbla), out=out, orbit=orbit, bla=bla,
                            xbla=xbla)

    def launch_render_view(self, view: View, mrd: int, *, palette, d_rgba: int, source: str = "smooth", supersample: int = 1,
                           stream: int = 0, window=None, kernel: str = "default", max_band_rows: int = 0, lut=None) -> None:
        """Asynchronous render into a DEVICE buffer of nrows * ncols * 4 bytes (e.g. a torch tensor's data_ptr()) on
        ``stream`` (0 = HIP's null stream).  Source "equalized" with lut=None first takes the whole view's histogram
        synchronously (view_histogram), as render_view does."""
        self._render("launch", view, mrd, palette, source, supersample, window, max_band_rows, lut,
                     lambda: self.view_histogram(view, mrd, kernel=kernel), d_rgba=d_rgba, stream=stream, kernel=kernel)

    def launch_render_deep_view(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, d_rgba: int,
                                source: str = "smooth", supersample: int = 1, stream: int = 0, window=None,
                                max_band_rows: int = 0, lut=None, bla: bool = False, xbla: bool = False) -> None:
        self._render("launch", view, mrd, palette, source, supersample, window, max_band_rows, lut,
                     lambda: self.deep_view_histogram(orbit, view, mrd, bla=bla, xbla=xbla), d_rgba=d_rgba, stream=stream, orbit=orbit,
                     bla=bla, xbla=xbla)

    # -- adaptive supersampling (include/mbk.h, "Adaptive supersampling"): plain views, source "smooth" --
    def render_view_adaptive(self, view: View, mrd: int, *, palette, supersample: int, threshold: int, window=None,
                             kernel: str = "default", max_band_rows: int = 0, out: Optional[np.ndarray] = None,
                             want_mask: bool = False):
        """render_view(source="smooth") that computes the s x s samples only where they change the picture: a pixel is refined
        when its s = 1 colour differs from one of its up to eight neighbours' in the whole view by `threshold` (0 .. 256) or
        more in some channel, and is its s = 1 colour otherwise.  threshold 0 is render_view at `supersample` bit for bit,
        256 is render_view at 1.  Returns (rgba uint8[nrows, ncols, 4], TileStats over the samples computed for the window's
        pixels), or with want_mask (rgba, mask uint8[nrows, ncols] -- 1 where refined --, TileStats)."""
        cv = self._cview(view, window)
        rgba = self._render_out(cv, out)
        mask = np.empty((cv.nrows, cv.ncols), np.uint8) if want_mask else None
        spec = palette.spec("smooth", supersample, max_band_rows)
        st = L.mbk_stats()
        self._check(self._lib.mbk_view_render_adaptive_compute(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                               int(threshold), rgba.ctypes.data,
                                                               mask.ctypes.data if want_mask else None, C.byref(st)))
        return (rgba, mask, _stats(st)) if want_mask else (rgba, _stats(st))

    def launch_render_view_adaptive(self, view: View, mrd: int, *, palette, supersample: int, threshold: int, d_rgba: int,
                                    d_mask: int = 0, stream: int = 0, window=None, kernel: str = "default",
                                    max_band_rows: int = 0) -> None:
        """Asynchronous form into a DEVICE buffer of nrows * ncols * 4 bytes and, with d_mask, a DEVICE mask of nrows * ncols
        bytes, on ``stream`` (0 = HIP's null stream).  Nothing of the list of refined pixels reaches the host."""
        cv = self._cview(view, window)
        spec = palette.spec("smooth", supersample, max_band_rows)
        self._check(self._lib.mbk_view_render_adaptive_launch(self._h, C.byref(cv), mrd, L.KERNELS[kernel], C.byref(spec),
                                                              int(threshold), d_rgba or None, d_mask or None, stream or None))

    # -- adaptive supersampling of deep views (include/mbk.h, the section of that name): a DeepView, source "smooth" --
    @staticmethod
    def _adaptive_deep(view) -> None:
        if not isinstance(view, DeepView):
            raise ValueError("render_deep_view_adaptive takes a DeepView (a WideDeepView: render_wide_view_adaptive)")

    def render_deep_view_adaptive(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, supersample: int, threshold: int,
                                  window=None, max_band_rows: int = 0, out: Optional[np.ndarray] = None, want_mask: bool = False,
                                  bla: bool = False):
        """render_view_adaptive for a deep view: render_deep_view(source="smooth") that computes the s x s samples only for the
        pixels whose s = 1 colour differs from a neighbour's by `threshold` or more.  threshold 0 is render_deep_view at
        `supersample` bit for bit, 256 is render_deep_view at 1.  bla: both kinds of sample are those of
        compute_deep_view(bla=True), each with the table of its own view (W x H, and s times that); the first call with a
        given (orbit, view, supersample) builds and uploads what is missing of the two.  Returns (rgba, TileStats) or, with
        want_mask, (rgba, mask, TileStats), as render_view_adaptive."""
        self._adaptive_deep(view)
        cv = self._cdeep(view, window)
        rgba = self._render_out(cv, out)
        mask = np.empty((cv.nrows, cv.ncols), np.uint8) if want_mask else None
        spec = palette.spec("smooth", supersample, max_band_rows)
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_view_render_adaptive_compute(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_BLA if bla else 0,
                                                                    C.byref(spec), int(threshold), rgba.ctypes.data,
                                                                    mask.ctypes.data if want_mask else None, C.byref(st)))
        return (rgba, mask, _stats(st)) if want_mask else (rgba, _stats(st))

    def launch_render_deep_view_adaptive(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, palette, supersample: int,
                                         threshold: int, d_rgba: int, d_mask: int = 0, stream: int = 0, window=None,
                                         max_band_rows: int = 0, bla: bool = False) -> None:
        """Asynchronous form into a DEVICE buffer of nrows * ncols * 4 bytes and, with d_mask, a DEVICE mask of nrows * ncols
        bytes, on ``stream`` (0 = HIP's null stream).  With bla the first launch of an (orbit, view, supersample) builds and
        uploads its tables synchronously; later ones wait for nothing while both stay resident."""
        self._adaptive_deep(view)
        cv = self._cdeep(view, window)
        spec = palette.spec("smooth", supersample, max_band_rows)
        self._check(self._lib.mbk_deep_view_render_adaptive_launch(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_BLA if bla else 0,
                                                                   C.byref(spec), int(threshold), d_rgba or None, d_mask or None,
                                                                   stream or None))

    # -- adaptive supersampling of extended-range deep views (include/mbk.h, the section of that name): a WideDeepView --
    @staticmethod
    def _adaptive_wide(view) -> None:
        if not isinstance(view, WideDeepView):
            raise ValueError("render_wide_view_adaptive takes a WideDeepView (a DeepView: render_deep_view_adaptive)")

    def render_wide_view_adaptive(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, supersample: int, threshold: int,
                                  window=None, max_band_rows: int = 0, out: Optional[np.ndarray] = None, want_mask: bool = False,
                                  xbla: bool = False):
        """render_deep_view_adaptive for a WideDeepView: render_deep_view(wide_view, source="smooth") that computes the s x s
        samples only for the pixels whose s = 1 colour differs from a neighbour's by `threshold` or more.  threshold 0 is
        render_deep_view at `supersample` bit for bit, 256 is render_deep_view at 1.  xbla: both kinds of sample are those of
        compute_deep_view(xbla=True), each with the table of its own view (W x H, and s times that); the first call with a
        given (orbit, view, supersample) builds and uploads what is missing of the two.  Returns (rgba, TileStats) or, with
        want_mask, (rgba, mask, TileStats), as render_view_adaptive."""
        self._adaptive_wide(view)
        cv = self._cdeep(view, window)
        rgba = self._render_out(cv, out)
        mask = np.empty((cv.nrows, cv.ncols), np.uint8) if want_mask else None
        spec = palette.spec("smooth", supersample, max_band_rows)
        st = L.mbk_stats()
        self._check(self._lib.mbk_deep_xview_render_adaptive_compute(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_XBLA if xbla else 0,
                                                                     C.byref(spec), int(threshold), rgba.ctypes.data,
                                                                     mask.ctypes.data if want_mask else None, C.byref(st)))
        return (rgba, mask, _stats(st)) if want_mask else (rgba, _stats(st))

    def launch_render_wide_view_adaptive(self, orbit: DeepOrbit, view: WideDeepView, mrd: int, *, palette, supersample: int,
                                         threshold: int, d_rgba: int, d_mask: int = 0, stream: int = 0, window=None,
                                         max_band_rows: int = 0, xbla: bool = False) -> None:
        """Asynchronous form into a DEVICE buffer of nrows * ncols * 4 bytes and, with d_mask, a DEVICE mask of nrows * ncols
        bytes, on ``stream`` (0 = HIP's null stream).  The first launch of an (orbit, view, supersample) uploads the wide orbit
        table and, with xbla, builds and uploads its tables synchronously; later ones wait for nothing while both stay
        resident."""
        self._adaptive_wide(view)
        cv = self._cdeep(view, window)
        spec = palette.spec("smooth", supersample, max_band_rows)
        self._check(self._lib.mbk_deep_xview_render_adaptive_launch(self._h, orbit._h, C.byref(cv), mrd, L.MBK_DEEP_XBLA if xbla else 0,
                                                                    C.byref(spec), int(threshold), d_rgba or None, d_mask or None,
                                                                    stream or None))

    # -- count histograms (include/mbk.h, "Count histograms and histogram-equalised colouring") ------
    def view_histogram(self, view: View, mrd: int, *, window=None, kernel: str = "default", precision: str = "f64",
                       want_stats: bool = False):
        """The histogram of the window's escape counts, built on the GPU: uint64[mrd], hist[c] the number of samples whose
        count is c.  Only 8 * mrd bytes cross PCIe.  want_stats: (hist, TileStats) -- never_pixels and pixel_iterations from
        the reduction over the same counts, hist[0] and sum c hist[c] + (mrd - 1) hist[0]."""
        return self._histogram(view, mrd, window, want_stats, kernel=kernel, precision=precision)

    def deep_view_histogram(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, window=None, want_stats: bool = False,
                            bla: bool = False, xbla: bool = False):
        """view_histogram for a deep view (bla / xbla: of the counts of compute_deep_view with the same keyword)."""
        return self._histogram(view, mrd, window, want_stats, orbit=orbit, bla=bla, xbla=xbla)

    def launch_view_histogram(self, view: View, mrd: int, *, d_hist: int, stream: int = 0, window=None, kernel: str = "default",
                              precision: str = "f64") -> None:
        """Asynchronous form: the window's histogram is ADDED into the DEVICE table d_hist (uint64[mrd]; the caller clears it)
        on ``stream`` (0 = HIP's null stream)."""
        self._launch_histogram(view, mrd, d_hist, stream, window, kernel=kernel, precision=precision)

    def launch_deep_view_histogram(self, orbit: DeepOrbit, view: DeepView, mrd: int, *, d_hist: int, stream: int = 0,
                                   window=None, bla: bool = False, xbla: bool = False) -> None:
        self._launch_histogram(view, mrd, d_hist, stream, window, orbit=orbit, bla=bla, xbla=xbla)

    def counts_histogram(self, d_counts: int, n: int, mrd: int, d_hist: int, stream: int = 0) -> None:
        """Asynchronous: the histogram of n int32 counts in DEVICE memory is ADDED into the DEVICE table d_hist (uint64[mrd])
        on ``stream``; counts outside [0, mrd - 1] are skipped.  The sibling of reduce_counts."""
        self._check(self._lib.mbk_counts_histogram(self._h, d_counts or None, n, mrd, d_hist or None, stream or None))

    # -- density views (include/mbk.h, "Density views") -------------------------------------------------
    def compute_view_density(self, view: View, target: DensityTarget, mrd: int, *, min_count: int = 1, max_count: int = 0,
                             window=None, kernel: str = "default", out: Optional[np.ndarray] = None):
        """The Buddhabrot density of the view's samples: every sample whose count n lies in [min_count, max_count]
        (max_count 0: mrd - 1) deposits its n orbit points z_0 .. z_(n-1) into the cells of `target`.  Synchronous; only the
        table crosses PCIe.  Returns (table uint32[height, width] -- overwritten, not accumulated --, TileStats over the
        samples, DensityStats)."""
        cv = self._cview(view, window)
        ct = target.ctarget()
        shape = (max(int(target.height), 0), max(int(target.width), 0))
        table = _out_array(out, shape, np.uint32)
        st, ds = L.mbk_stats(), L.mbk_density_stats()
        self._check(self._lib.mbk_view_density_compute(self._h, C.byref(cv), C.byref(ct), mrd, min_count, max_count, L.KERNELS[kernel],
                                                       table.ctypes.data if table.size else None, C.byref(st), C.byref(ds)))
        return table.reshape(shape), _stats(st), DensityStats(int(ds.deposits), int(ds.dropped))

    def launch_view_density(self, view: View, target: DensityTarget, mrd: int, *, d_density: int, min_count: int = 1,
                            max_count: int = 0, stream: int = 0, window=None, kernel: str = "default") -> None:
        """Asynchronous form: the window's deposits are ADDED into the DEVICE table d_density (uint32[height * width]; the
        caller clears it) on ``stream`` (0 = HIP's null stream), so that windows, bands and launches accumulate."""
        cv = self._cview(view, window)
        ct = target.ctarget()
        self._check(self._lib.mbk_view_density_launch(self._h, C.byref(cv), C.byref(ct), mrd, min_count, max_count, L.KERNELS[kernel],
                                                      d_density or None, stream or None))

    def density_max(self, d_density: int, n: int, stream: int = 0) -> Tuple[int, int]:
        """(max, total) of n cells of a DEVICE table, reduced on the GPU on ``stream`` (the call waits for that stream)."""
        mx, total = C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.mbk_density_max(self._h, d_density or None, n, C.byref(mx), C.byref(total), stream or None))
        return int(mx.value), int(total.value)

    def render_density(self, table: np.ndarray, *, palette, mode: str = "sqrt", factor: int = 1, out: Optional[np.ndarray] = None):
        """A HOST density table (uint32[height, width]) as an RGBA8 image of (height / factor, width / factor) pixels, coloured
        (image.Palette.for_density) and box-filtered on the GPU.  Returns (rgba uint8[h, w, 4], TileStats)."""
        t = np.ascontiguousarray(table, dtype=np.uint32)
        if t.ndim != 2:
            raise ValueError("a density table is a (height, width) uint32 array")
        h, w = t.shape
        k = int(factor) if factor in L.DENSITY_FACTORS else 1   # (a bad factor is refused by the library)
        shape = (h // k, w // k, 4)
        rgba = _out_array(out, shape, np.uint8).reshape(shape)
        spec = palette.density_spec(mode, factor)
        st = L.mbk_stats()
        self._check(self._lib.mbk_density_render_compute(self._h, t.ctypes.data if t.size else None, w, h, C.byref(spec),
                                                         rgba.ctypes.data if rgba.size else None, C.byref(st)))
        return rgba, _stats(st)

    def launch_render_density(self, d_density: int, width: int, height: int, *, palette, d_rgba: int, mode: str = "sqrt",
                              factor: int = 1, stream: int = 0) -> None:
        """Asynchronous render of a DEVICE table into a DEVICE image of (height / factor) * (width / factor) * 4 bytes on
        ``stream`` (0 = HIP's null stream)."""
        spec = palette.density_spec(mode, factor)
        self._check(self._lib.mbk_density_render_launch(self._h, d_density or None, width, height, C.byref(spec), d_rgba or None,
                                                        stream or None))

    # -- Julia views (include/mbk.h, "Julia views") ---------------------------------------------------
    def compute_julia_view(self, view: View, c, mrd: int, *, window=None, want_counts: bool = True, want_bytes: bool = True,
                           want_smooth: bool = False, kernel: str = "default", out_counts: Optional[np.ndarray] = None,
                           out_bytes: Optional[np.ndarray] = None):
        """The Julia set of the parameter c = (c_r, c_i) on `view`: z -> z^2 + c from z_0 = the pixel's coordinate.
        Synchronous: (counts int32 | None, bytes uint8 | None, smooth float64 | None, TileStats), each [nrows, ncols].
        kernel: "default", "asm" (the per-step loop) or "group"."""
        cv = self._cview(view, window)
        shape = (cv.nrows, cv.ncols)
        counts = _out_array(out_counts, shape, np.int32) if want_counts else None
        byts = _out_array(out_bytes, shape, np.uint8) if want_bytes else None
        smooth = np.empty(shape, np.float64) if want_smooth else None
        flags, p_counts, p_bytes = _wanted(shape, counts, byts)
        st = L.mbk_stats()
        self._check(self._lib.mbk_julia_view_compute(self._h, C.byref(cv), float(c[0]), float(c[1]), mrd, L.KERNELS[kernel] | flags,
                                                     p_counts, p_bytes, smooth.ctypes.data if smooth is not None else None,
                                                     C.byref(st)))
        return counts, byts, smooth, _stats(st)

    def submit_julia_view(self, slot: int, view: View, c, mrd: int, *, window=None, out_counts: Optional[np.ndarray] = None,
                          out_bytes: Optional[np.ndarray] = None, kernel: str = "default") -> None:
        """Enqueue a Julia view / window on `slot`; the host arrays are valid after wait(slot)."""
        cv = self._cview(view, window)
        flags, p_counts, p_bytes = _wanted((cv.nrows, cv.ncols), out_counts, out_bytes)
        self._check(self._lib.mbk_julia_view_submit(self._h, slot, C.byref(cv), float(c[0]), float(c[1]), mrd,
                                                    L.KERNELS[kernel] | flags, p_counts, p_bytes))

    def launch_julia_view(self, view: View, c, mrd: int, *, d_counts: int = 0, d_bytes: int = 0, d_smooth: int = 0,
                          stream: int = 0, window=None, kernel: str = "default") -> None:
        """Asynchronous launch on raw DEVICE pointers on ``stream`` (0 = HIP's null stream)."""
        cv = self._cview(view, window)
        flags = L.KERNELS[kernel] | (L.MBK_WANT_COUNTS if d_counts else 0) | (L.MBK_WANT_BYTES if d_bytes else 0)
        self._check(self._lib.mbk_julia_view_launch(self._h, C.byref(cv), float(c[0]), float(c[1]), mrd, flags, d_counts or None,
                                                    d_bytes or None, d_smooth or None, stream or None))

    def render_julia_view(self, view: View, c, mrd: int, *, palette, source: str = "smooth", supersample: int = 1, window=None,
                          kernel: str = "default", max_band_rows: int = 0, out: Optional[np.ndarray] = None, lut=None):
        """render_view for the Julia set of c: source "bytes", "smooth" or "equalized" (`lut` as for render_view: None takes
        the table of julia_view_histogram of the whole view); the distance sources are refused (MbkError)."""
        return self._render("compute", view, mrd, palette, source, supersample, window, max_band_rows, lut,
                            lambda: self.julia_view_histogram(view, c, mrd, kernel=kernel), out=out, c=c, kernel=kernel)

    def launch_render_julia_view(self, view: View, c, mrd: int, *, palette, d_rgba: int, source: str = "smooth",
                                 supersample: int = 1, stream: int = 0, window=None, kernel: str = "default",
                                 max_band_rows: int = 0, lut=None) -> None:
        """Asynchronous render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream``; "equalized" with lut=None first
        takes the whole view's histogram synchronously, as render_julia_view does."""
        self._render("launch", view, mrd, palette, source, supersample, window, max_band_rows, lut,
                     lambda: self.julia_view_histogram(view, c, mrd, kernel=kernel), d_rgba=d_rgba, stream=stream, c=c, kernel=kernel)

    def julia_view_histogram(self, view: View, c, mrd: int, *, window=None, kernel: str = "default", want_stats: bool = False):
        """view_histogram for the Julia set of c."""
        return self._histogram(view, mrd, window, want_stats, c=c, kernel=kernel)

    def launch_julia_view_histogram(self, view: View, c, mrd: int, *, d_hist: int, stream: int = 0, window=None,
                                    kernel: str = "default") -> None:
        """Asynchronous form: the window's histogram is ADDED into the DEVICE table d_hist (uint64[mrd]) on ``stream``."""
        self._launch_histogram(view, mrd, d_hist, stream, window, c=c, kernel=kernel)

    # -- distance estimates for Julia views (include/mbk.h, the section of that name): calls of their own; render_julia_view
    # keeps refusing the distance sources --
    def compute_julia_view_distance(self, view: View, c, mrd: int, *, window=None, kernel: str = "default"):
        """Exterior distance estimates of the Julia set of c: de = 2 |z| ln |z| / |dz/dz_0| in complex-plane units, evaluated
        after the orbit has run on to |z|^2 >= 2^32, 0 for never-escaped pixels.  The counts are those of compute_julia_view.
        kernel "asm" takes the one-pass form; "default" and "group" compute the counts with that kernel first and the
        derivative in a second pass; all store the same values.  A pixel at exactly 0 (the critical point) that escapes has
        derivative 0 and stores +inf.  Returns (distance float64[nrows,ncols], counts int32[nrows,ncols], TileStats)."""
        return self._distance_values("compute", "julia", view, mrd, window, c=c, kernel=kernel)

    def launch_julia_view_distance(self, view: View, c, mrd: int, *, d_distance: int, d_counts: int = 0, stream: int = 0,
                                   window=None, kernel: str = "default") -> None:
        """Asynchronous form on DEVICE pointers (float64 / int32 of the window's size) on ``stream`` (0 = HIP's null stream)."""
        self._distance_values("launch", "julia", view, mrd, window, d_values=d_distance, d_counts=d_counts, stream=stream, c=c, kernel=kernel)

    def render_julia_view_distance(self, view: View, c, mrd: int, *, palette, supersample: int = 1, window=None,
                                   kernel: str = "default", max_band_rows: int = 0, out: Optional[np.ndarray] = None):
        """The Julia set of c as an RGBA8 image coloured by its distance estimate (source "distance"; Palette.distance), as
        render_view(source="distance") does for a plain view.  Returns (rgba uint8[nrows, ncols, 4], TileStats)."""
        return self._distance_render("compute", "julia", view, mrd, palette, supersample, window, max_band_rows, out=out, c=c, kernel=kernel)

    def launch_render_julia_view_distance(self, view: View, c, mrd: int, *, palette, d_rgba: int, supersample: int = 1,
                                          stream: int = 0, window=None, kernel: str = "default", max_band_rows: int = 0) -> None:
        """Asynchronous render into a DEVICE buffer of nrows * ncols * 4 bytes on ``stream`` (0 = HIP's null stream)."""
        self._distance_render("launch", "julia", view, mrd, palette, supersample, window, max_band_rows, d_rgba=d_rgba, stream=stream, c=c,
                              kernel=kernel)

    # -- stored chunks (include/mbk.h, "Stored chunks") ---------------------------------------------
    def decode_chunk(self, stream, n: int = L.MBK_CHUNK_BYTES, out: Optional[np.ndarray] = None):
        """A chunk stream (what DataChunk.Serialize writes / a DataServer sends) decoded on the GPU: (uint8[n], TileStats).
        The statistics are those of the decoded bytes (all_bytes_zero / all_bytes_one, rle_runs).  MbkError for an invalid
        stream, with `out` untouched."""
        a = _stream_array(stream)
        out = _out_array(out, n, np.uint8)
        st = L.mbk_stats()
        self._check(self._lib.mbk_chunk_decode_compute(self._h, _stream_ptr(a), a.size,
                                                       n, out.ctypes.data, C.byref(st)))
        return out, _stats(st)

    @staticmethod
    def _chunk_spec(palette, scale: int) -> L.mbk_chunk_spec:
        if len(palette) != 256:
            raise ValueError("a chunk is coloured through a palette of 256 entries")
        return L.mbk_chunk_spec(palette.entries.ctypes.data, int(scale))

    def render_chunk(self, stream, *, palette=None, scale: int = 1, out: Optional[np.ndarray] = None,
                     pitch: Optional[int] = None):
        """A stored 4096 x 4096 chunk as an RGBA8 image of (4096 / scale)^2 pixels, decoded, coloured (palette[byte]; default
        the reference Viewer's colouring) and box-filtered on the GPU.  `out` may be a (pinned) uint8 array -- or a view
        into a larger image: then `pitch` is the distance of its rows in pixels, and the chunk lands at out's first
        element.  Returns (uint8[h, w, 4] -- a view into `out` if given --, TileStats); row 0 is the lowest imaginary part."""
        from .image import Palette
        palette = Palette.viewer() if palette is None else palette
        a = _stream_array(stream)
        w = L.MBK_CHUNK_DEFINITION // int(scale) if scale in L.CHUNK_SCALES else 0
        if out is None:
            out = np.empty((w, w, 4), np.uint8)
            pitch = w
        else:
            pitch = w if pitch is None else int(pitch)
            if out.dtype != np.uint8 or (w and out.ndim == 3 and out.strides != (4 * pitch, 4, 1)):
                raise ValueError("out must be uint8 rows of 4-byte pixels, `pitch` pixels apart")
        spec = self._chunk_spec(palette, scale)
        st = L.mbk_stats()
        self._check(self._lib.mbk_chunk_render_compute(self._h, _stream_ptr(a), a.size,
                                                       C.byref(spec), out.ctypes.data, pitch, C.byref(st)))
        return out, _stats(st)

    def launch_decode_chunk(self, stream, *, d_bytes: int, n: int = L.MBK_CHUNK_BYTES, d_status: int = 0,
                            hip_stream: int = 0) -> None:
        """Asynchronous decode into a DEVICE buffer of n bytes on ``hip_stream`` (0 = HIP's null stream); the reason code goes
        to the device word d_status.  `stream` must stay alive until the HIP stream has passed the copy; a uint8 array over
        pinned memory (`pinned_empty`) makes the copy asynchronous."""
        a = _stream_array(stream)
        self._check(self._lib.mbk_chunk_decode_launch(self._h, _stream_ptr(a), a.size, n,
                                                      d_bytes or None, d_status or None, hip_stream or None))

    def launch_render_chunk(self, stream, *, d_rgba: int, palette=None, scale: int = 1, pitch: Optional[int] = None,
                            d_status: int = 0, hip_stream: int = 0) -> None:
        """Asynchronous render into a DEVICE image on ``hip_stream``: the chunk's pixel (x, y) at d_rgba + 4 (y pitch + x)."""
        from .image import Palette
        palette = Palette.viewer() if palette is None else palette
        a = _stream_array(stream)
        spec = self._chunk_spec(palette, scale)
        w = L.MBK_CHUNK_DEFINITION // int(scale) if scale in L.CHUNK_SCALES else 0
        self._check(self._lib.mbk_chunk_render_launch(self._h, _stream_ptr(a), a.size,
                                                      C.byref(spec), d_rgba or None, w if pitch is None else int(pitch),
                                                      d_status or None, hip_stream or None))

    def reduce_counts(self, d_counts: int, n: int, mrd: int, stream: int = 0) -> TileStats:
        st = L.mbk_stats()
        self._check(self._lib.mbk_reduce_counts(self._h, d_counts, n, mrd, stream or None, C.byref(st)))
        return _stats(st)


def _stats(st: L.mbk_stats) -> TileStats:
    return TileStats(float(st.kernel_ms), float(st.d2h_ms), int(st.pixel_iterations),
                     int(st.never_pixels), bool(st.all_bytes_zero), bool(st.all_bytes_one), int(st.rle_runs))


def render_adaptive_host(palette, supersample: int, threshold: int, width: int, height: int, *, base_counts, base_smooth,
                         fine_counts, fine_smooth, want_mask: bool = False):
    """mbk_render_adaptive_host: the adaptive-supersampling contract on the host, no device -- the same functions the kernels are
    compiled from.  base_*: the samples of the FULL (height, width) view; fine_*: those of the FULL (height s, width s) view.
    Returns rgba uint8[height, width, 4], or with want_mask (rgba, mask uint8[height, width])."""
    lib = L.load()
    s = int(supersample)
    arrs = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((base_counts, np.int32), (base_smooth, np.float64),
                                                            (fine_counts, np.int32), (fine_smooth, np.float64))]
    for a, n in zip(arrs, (width * height, width * height, width * height * s * s, width * height * s * s)):
        if a.size != n:
            raise ValueError("base arrays hold height x width samples, fine arrays (height * s) x (width * s)")
    rgba = np.empty((height, width, 4), np.uint8)
    mask = np.empty((height, width), np.uint8) if want_mask else None
    spec = palette.spec("smooth", s)
    _check(lib, lib.mbk_render_adaptive_host(C.byref(spec), int(threshold), width, height, *[a.ctypes.data for a in arrs],
                                             rgba.ctypes.data, mask.ctypes.data if want_mask else None))
    return (rgba, mask) if want_mask else rgba
