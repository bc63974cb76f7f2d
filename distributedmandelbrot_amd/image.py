"""Palettes for MandelbrotDevice.render_view / render_deep_view (include/mbk.h, "Rendering") and a PNG writer.

Nothing here needs a GPU, and no imaging library is imported: the PNG writer is zlib + struct.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib as L


@dataclass(frozen=True)
class Palette:
    """n RGBA8 entries plus, for source "smooth", the colour of never-escaping samples and the map from the smooth value
    nu to a palette position, t = nu * scale + offset (entries are blended linearly and the palette is cyclic).
    Source "bytes" takes 256 entries, indexed by the quantised byte; `inside`, `scale` and `offset` are not used there.
    Source "distance" maps the distance estimate de the same way, t = de * scale + offset, but the palette does not wrap:
    t >= n - 1 is the last entry (Palette.distance / for_distance set scale from a view's pixel pitch).  Source "distance_rel"
    (deep views) does the same with the distance as a fraction of the view's span (Palette.deep_distance / for_deep_distance).
    Source "equalized" maps v in [0, 1], nu sent through an equalisation table (equalize_lut), without a wrap as well
    (Palette.for_equalized spreads the whole palette over it)."""
    entries: np.ndarray
    inside: Tuple[int, int, int, int] = (0, 0, 0, 255)
    scale: float = 1.0
    offset: float = 0.0

    def __post_init__(self):
        e = np.ascontiguousarray(self.entries, dtype=np.uint8)
        if e.ndim != 2 or e.shape[1] != 4:
            raise ValueError("a palette is an (n, 4) uint8 array of RGBA entries")
        object.__setattr__(self, "entries", e)
        object.__setattr__(self, "inside", tuple(int(v) for v in self.inside))

    def __len__(self) -> int:
        return int(self.entries.shape[0])

    @staticmethod
    def viewer() -> "Palette":
        """The reference Viewer's colouring of a chunk's bytes (DistributedMandelbrotViewer.py:110-135): black for byte 0,
        jet(1 - b / 256) otherwise -- mbk_palette_viewer."""
        out = np.empty((256, 4), np.uint8)
        st = L.load().mbk_palette_viewer(out.ctypes.data)
        if st != L.MBK_OK:
            raise RuntimeError(f"mbk_palette_viewer failed with status {st}")
        return Palette(out)

    @staticmethod
    def cosine(n: int = 1024, *, phase=(0.0, 0.33, 0.67), period: float = 32.0, inside=(0, 0, 0, 255)) -> "Palette":
        """A cyclic palette of n entries, channel c = 0.5 - 0.5 cos(2 pi (k / n + phase[c])); one turn of the palette spans
        `period` units of nu."""
        k = np.arange(n, dtype=np.float64)[:, None] / n
        rgb = 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + np.asarray(phase, np.float64)[None, :]))
        e = np.empty((n, 4), np.uint8)
        e[:, :3] = np.floor(255.0 * rgb + 0.5).astype(np.uint8)
        e[:, 3] = 255
        return Palette(e, inside=inside, scale=n / float(period))

    @staticmethod
    def gradient(stops, n: int = 1024, *, period: float = 32.0, inside=(0, 0, 0, 255)) -> "Palette":
        """A cyclic palette of n entries that runs linearly through the RGB `stops` and back to the first one."""
        s = np.asarray(list(stops) + [stops[0]], np.float64)
        x = np.arange(n, dtype=np.float64) * (len(s) - 1) / n
        e = np.empty((n, 4), np.uint8)
        for c in range(3):
            e[:, c] = np.floor(np.interp(x, np.arange(len(s)), s[:, c]) + 0.5).astype(np.uint8)
        e[:, 3] = 255
        return Palette(e, inside=inside, scale=n / float(period))

    def for_distance(self, view, width_px: float, *, inner_px: float = 0.0) -> "Palette":
        """This palette stretched over distances of inner_px .. width_px OUTPUT pixels of `view` for source "distance":
        scale = (n - 1) / ((width_px - inner_px) pitch), pitch the view's sample spacing (range_r / (width - 1)), and
        offset = -inner_px (n - 1) / (width_px - inner_px).  Samples nearer than inner_px take entry 0, samples beyond
        width_px the last entry."""
        if not width_px > inner_px >= 0.0:
            raise ValueError("0 <= inner_px < width_px")
        if view.width > 1:
            pitch = abs(view.range_r) / (view.width - 1)
        else:
            pitch = abs(view.range_i) / max(view.height - 1, 1)
        if not pitch > 0.0:
            raise ValueError("the view has no pixel pitch")
        span = float(width_px) - float(inner_px)
        return Palette(self.entries, self.inside, (len(self) - 1) / (span * pitch), -float(inner_px) * (len(self) - 1) / span)

    @staticmethod
    def distance(view, width_px: float = 8.0, *, inner_px: float = 0.0, near=(0, 0, 0), far=(255, 255, 255), n: int = 256,
                 inside=(0, 0, 0, 255)) -> "Palette":
        """A ramp of n entries from `near` to `far` for source "distance": `near` within inner_px output pixels of the set,
        `far` beyond width_px -- Palette.distance(view, 8, inner_px=1) is black within 1 px of the set and white beyond 8."""
        return Palette(Palette._ramp(near, far, n), inside=inside).for_distance(view, width_px, inner_px=inner_px)

    def for_deep_distance(self, view, width_px: float, *, inner_px: float = 0.0) -> "Palette":
        """for_distance for a DeepView or a WideDeepView and source "distance_rel", whose samples are fractions of the view's real span: one
        OUTPUT pixel is 1 / (width - 1) of it, so scale = (n - 1) (width - 1) / (width_px - inner_px) and
        offset = -inner_px (n - 1) / (width_px - inner_px), whatever the span and the supersampling factor."""
        if not width_px > inner_px >= 0.0:
            raise ValueError("0 <= inner_px < width_px")
        if view.width > 1:
            per_px = float(view.width - 1)
        elif hasattr(view, "range_r"):   # a WideDeepView's single column: the common 2^exp2 cancels
            per_px = max(view.height - 1, 1) * (view.range_r / view.range_i)
        else:   # a single column: the rows' pitch, in units of span_r
            per_px = max(view.height - 1, 1) * (view.span_r / view.span_i)
        span = float(width_px) - float(inner_px)
        return Palette(self.entries, self.inside, (len(self) - 1) * per_px / span, -float(inner_px) * (len(self) - 1) / span)

    @staticmethod
    def deep_distance(view, width_px: float = 8.0, *, inner_px: float = 0.0, near=(0, 0, 0), far=(255, 255, 255), n: int = 256,
                      inside=(0, 0, 0, 255)) -> "Palette":
        """Palette.distance for a DeepView and source "distance_rel"."""
        return Palette(Palette._ramp(near, far, n), inside=inside).for_deep_distance(view, width_px, inner_px=inner_px)

    def for_equalized(self) -> "Palette":
        """This palette spread over the equalised value v in [0, 1] of source "equalized": scale = n - 1, offset = 0, so that
        equal shares of the escaped samples take equal stretches of the palette."""
        return Palette(self.entries, self.inside, float(len(self) - 1), 0.0)

    def for_density(self, max_value: float, mode: str = "sqrt") -> "Palette":
        """This palette stretched over a density table whose largest cell is `max_value` (MandelbrotDevice.density_max), for
        render_density with the same `mode`: scale = (n - 1) / g(max_value), offset = 0, so that g(max_value) reaches the last
        entry (g(v) = sqrt(v) for "sqrt", v for "linear").  The scale is nudged up by ulps where rounding would leave
        fl(g scale) just below n - 1."""
        if mode not in L.DENSITY_MODES:
            raise ValueError("mode must be 'sqrt' or 'linear'")
        if not max_value >= 1:
            raise ValueError("max_value must be at least 1")
        g = float(np.sqrt(np.float64(max_value))) if mode == "sqrt" else float(max_value)
        last = float(len(self) - 1)
        scale = last / g
        while g * scale < last:
            scale = float(np.nextafter(scale, np.inf))
        return Palette(self.entries, self.inside, scale, 0.0)

    def density_spec(self, mode: str, factor: int) -> L.mbk_density_render_spec:
        """The C struct of a density render; it points into self.entries, which the caller keeps alive for the call."""
        return L.mbk_density_render_spec(L.DENSITY_MODES[mode], int(factor), self.entries.ctypes.data, len(self),
                                         float(self.scale), float(self.offset))

    def relief_spec(self, supersample: int, light_deg: float = 45.0, height: float = 1.5, max_band_rows: int = 0, *,
                    light=None) -> L.mbk_relief_spec:
        """The C struct of a relief render (include/mbk.h, "Relief shading"): this palette as for source "smooth", lit from
        the direction light_deg (degrees, counter-clockwise from the positive real axis) by a light `height` above the plane.
        light: the doubles (lx, ly) themselves in place of (cos, sin) of light_deg.  It points into self.entries, which the
        caller keeps alive for the call."""
        lx, ly = light if light is not None else (float(np.cos(np.deg2rad(light_deg))), float(np.sin(np.deg2rad(light_deg))))
        return L.mbk_relief_spec(int(supersample), self.entries.ctypes.data, len(self), (C.c_uint8 * 4)(*self.inside),
                                 float(self.scale), float(self.offset), float(lx), float(ly), float(height), int(max_band_rows))

    def stripe_spec(self, supersample: int, density: int = 5, skip: int = 0, lo: float = 0.35, gain: float = 1.0,
                    max_band_rows: int = 0) -> L.mbk_stripe_spec:
        """The C struct of a stripe render (include/mbk.h, "Stripe-average colouring"): this palette as for source "smooth",
        shaded by the stripe average of density `density` with the first `skip` orbit points left out; `lo` the brightness of
        the darkest stripe, `gain` the contrast.  It points into self.entries, which the caller keeps alive for the call."""
        return L.mbk_stripe_spec(int(supersample), self.entries.ctypes.data, len(self), (C.c_uint8 * 4)(*self.inside),
                                 float(self.scale), float(self.offset), int(density), int(skip), float(lo), float(gain),
                                 int(max_band_rows))

    @staticmethod
    def _ramp(near, far, n: int) -> np.ndarray:
        x = np.arange(n, dtype=np.float64)[:, None] / (n - 1)
        rgb = (1.0 - x) * np.asarray(near, np.float64)[None, :] + x * np.asarray(far, np.float64)[None, :]
        e = np.empty((n, 4), np.uint8)
        e[:, :3] = np.floor(rgb + 0.5).astype(np.uint8)
        e[:, 3] = 255
        return e

    def spec(self, source: str, supersample: int, max_band_rows: int = 0) -> L.mbk_render_spec:
        """The C struct; it points into self.entries, which the caller keeps alive for the call."""
        return L.mbk_render_spec(L.RENDER_SOURCES[source], int(supersample), self.entries.ctypes.data, len(self),
                                 (C.c_uint8 * 4)(*self.inside), float(self.scale), float(self.offset), int(max_band_rows))


def equalize_lut(hist) -> np.ndarray:
    """mbk_equalize_lut_host: the equalisation table, float64[mrd + 2], of a histogram of counts (uint64[mrd]; what
    MandelbrotDevice.view_histogram returns).  lut[k] is the share of escaped samples whose count is below k - 1 plus half the
    share with count k - 1; count 0 takes no part."""
    lib = L.load()
    h = np.ascontiguousarray(hist, dtype=np.uint64).ravel()
    lut = np.empty(h.size + 2, np.float64)
    st = lib.mbk_equalize_lut_host(h.ctypes.data if h.size else None, h.size, lut.ctypes.data)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return lut


def equalize_value(lut, nu: float) -> float:
    """mbk_equalize_value_host: the equalised value of one sample."""
    t = np.ascontiguousarray(lut, dtype=np.float64).ravel()
    return float(L.load().mbk_equalize_value_host(t.ctypes.data, t.size - 2, float(nu)))


def counts_histogram_host(counts, mrd: int, hist=None) -> np.ndarray:
    """mbk_counts_histogram_host: the histogram of int32 counts on the host, ADDED into `hist` (uint64[mrd]; None: zeros)."""
    lib = L.load()
    c = np.ascontiguousarray(counts, dtype=np.int32).ravel()
    hist = np.zeros(max(int(mrd), 0), np.uint64) if hist is None else hist
    assert hist.dtype == np.uint64 and hist.size == mrd and hist.flags.c_contiguous
    st = lib.mbk_counts_histogram_host(c.ctypes.data if c.size else None, c.size, mrd, hist.ctypes.data if hist.size else None)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return hist


def resolve_host(palette: Palette, source: str, supersample: int, width: int, height: int, *, counts=None, bytes_=None,
                 smooth=None, lut=None) -> np.ndarray:
    """mbk_render_resolve_host: colour and resolve caller-supplied samples of (height s, width s) on the host -- the same
    code the kernel is compiled from, without a device.  Source "equalized" takes the table `lut`
    (mbk_render_resolve_equalized_host)."""
    lib = L.load()
    out = np.empty((height, width, 4), np.uint8)
    arrs = []
    for a, dt in ((counts, np.int32), (bytes_, np.uint8), (smooth, np.float64)):
        arrs.append(None if a is None else np.ascontiguousarray(a, dtype=dt))
    for a in arrs:
        if a is not None and a.size != width * height * supersample * supersample:
            raise ValueError("sample arrays must hold (height * s) x (width * s) elements")
    spec = palette.spec(source, supersample)
    ptrs = [a.ctypes.data if a is not None else None for a in arrs]
    if lut is not None:
        t = np.ascontiguousarray(lut, dtype=np.float64).ravel()
        st = lib.mbk_render_resolve_equalized_host(C.byref(spec), t.ctypes.data, t.size, width, height, ptrs[0], ptrs[2],
                                                   out.ctypes.data)
    else:
        st = lib.mbk_render_resolve_host(C.byref(spec), width, height, *ptrs, out.ctypes.data)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return out


def relief_resolve_host(palette: Palette, supersample: int, width: int, height_px: int, *, counts, smooth, normals,
                        light_deg: float = 45.0, height: float = 1.5, light=None) -> np.ndarray:
    """mbk_relief_resolve_host: shade, colour and resolve caller-supplied samples of (height_px s, width s) on the host --
    counts, nu and normals[..., 2] -- with the code the relief resolve kernel is compiled from, without a device."""
    lib = L.load()
    out = np.empty((height_px, width, 4), np.uint8)
    c = np.ascontiguousarray(counts, dtype=np.int32)
    nu = np.ascontiguousarray(smooth, dtype=np.float64)
    nrm = np.ascontiguousarray(normals, dtype=np.float64)
    samples = width * height_px * supersample * supersample
    if c.size != samples or nu.size != samples or nrm.size != 2 * samples:
        raise ValueError("sample arrays must hold (height * s) x (width * s) elements, the normals two each")
    spec = palette.relief_spec(supersample, light_deg, height, light=light)
    st = lib.mbk_relief_resolve_host(C.byref(spec), width, height_px, c.ctypes.data, nu.ctypes.data, nrm.ctypes.data, out.ctypes.data)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return out


def stripe_resolve_host(palette: Palette, supersample: int, width: int, height_px: int, *, counts, smooth, stripe,
                        density: int = 5, skip: int = 0, lo: float = 0.35, gain: float = 1.0) -> np.ndarray:
    """mbk_stripe_resolve_host: shade, colour and resolve caller-supplied samples of (height_px s, width s) on the host --
    counts, nu and stripe averages -- with the code the stripe resolve kernel is compiled from, without a device."""
    lib = L.load()
    out = np.empty((height_px, width, 4), np.uint8)
    c = np.ascontiguousarray(counts, dtype=np.int32)
    nu = np.ascontiguousarray(smooth, dtype=np.float64)
    v = np.ascontiguousarray(stripe, dtype=np.float64)
    samples = width * height_px * supersample * supersample
    if c.size != samples or nu.size != samples or v.size != samples:
        raise ValueError("sample arrays must hold (height * s) x (width * s) elements")
    spec = palette.stripe_spec(supersample, density, skip, lo, gain)
    st = lib.mbk_stripe_resolve_host(C.byref(spec), width, height_px, c.ctypes.data, nu.ctypes.data, v.ctypes.data, out.ctypes.data)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return out


def resolve_density_host(palette: Palette, table, *, mode: str = "sqrt", factor: int = 1) -> np.ndarray:
    """mbk_density_resolve_host: a density table (uint32[height, width]) coloured and box-filtered on the host -- the same code
    the kernel is compiled from, without a device."""
    lib = L.load()
    t = np.ascontiguousarray(table, dtype=np.uint32)
    if t.ndim != 2:
        raise ValueError("a density table is a (height, width) uint32 array")
    h, w = t.shape
    k = int(factor) if factor in L.DENSITY_FACTORS else 1
    out = np.empty((h // k, w // k, 4), np.uint8)
    spec = palette.density_spec(mode, factor)
    st = lib.mbk_density_resolve_host(C.byref(spec), w, h, t.ctypes.data if t.size else None, out.ctypes.data if out.size else None)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return out


def resolve_chunk_host(palette: Palette, scale: int, bytes_, *, out=None, pitch=None) -> np.ndarray:
    """mbk_chunk_resolve_host: a decoded 4096 x 4096 chunk coloured through `palette` (256 entries) and box-filtered by
    `scale` on the host -- the same code the kernels are compiled from, without a device.  `out` / `pitch` as for
    MandelbrotDevice.render_chunk."""
    lib = L.load()
    b = np.ascontiguousarray(bytes_, dtype=np.uint8).ravel()
    if b.size != L.MBK_CHUNK_BYTES or len(palette) != 256:
        raise ValueError("a chunk holds 4096 x 4096 bytes and is coloured through 256 entries")
    w = L.MBK_CHUNK_DEFINITION // int(scale) if scale in L.CHUNK_SCALES else 0
    if out is None:
        out = np.empty((w, w, 4), np.uint8)
        pitch = w
    pitch = w if pitch is None else int(pitch)
    spec = L.mbk_chunk_spec(palette.entries.ctypes.data, int(scale))
    st = lib.mbk_chunk_resolve_host(C.byref(spec), b.ctypes.data, out.ctypes.data, pitch)
    if st != L.MBK_OK:
        from .device import MbkError
        raise MbkError(st, (lib.mbk_last_error(None) or b"").decode())
    return out


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, rgba: np.ndarray, *, flip: bool = True, level: int = 6) -> None:
    """Write an (h, w, 4) uint8 array as an 8-bit RGBA, non-interlaced PNG.  Row 0 of a render is the LOWEST imaginary part;
    PNG rows run top to bottom, so by default the rows are written in reverse (flip=False writes them as they are)."""
    a = np.asarray(rgba)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("write_png takes a non-empty (h, w, 4) uint8 array")
    if flip:
        a = a[::-1]
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 4 * w), np.uint8)   # filter type 0 in front of every row
    raw[:, 1:] = a.reshape(h, 4 * w)
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
