"""CPU tests of rendering (include/mbk.h, "Rendering"): the colour / resolve rule the resolve kernel is compiled from, run on
the host through mbk_render_resolve_host, against the numpy restatement of the contract (tests/render_model.py); the reference
Viewer's palette against the reference's recorded output; the PNG writer."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import render_model as M
from conftest import ROOT
from distributedmandelbrot_amd import MbkError, Palette, write_png
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.image import resolve_host

VIEWER_NPZ = os.path.join(ROOT, "tests", "golden", "viewer_palette.npz")
NEW_SYMBOLS = ["mbk_view_render_launch", "mbk_view_render_compute", "mbk_deep_view_render_launch",
               "mbk_deep_view_render_compute", "mbk_palette_viewer", "mbk_render_resolve_host"]


def _random_palette(rs, n):
    return Palette(rs.randint(0, 256, (n, 4)).astype(np.uint8), inside=tuple(rs.randint(0, 256, 4)),
                   scale=float(rs.choice([0.37, 1.0, 3.0, 41.7])), offset=float(rs.choice([0.0, -2.5, 0.125, 1000.75])))


def test_the_new_symbols_bind():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(L.mbk_render_spec) == 48 and L.mbk_render_spec.scale.offset == 24


def test_viewer_palette_equals_the_reference_viewers_output():
    """All 1024 bytes: the 8-bit form (floor(255 x + 0.5)) of what the reference's data_to_img_array returns per byte value
    (tests/golden/make_viewer_golden.py)."""
    z = np.load(VIEWER_NPZ)
    pal = Palette.viewer()
    assert pal.entries.shape == (256, 4)
    assert np.array_equal(pal.entries, z["rgba8"])
    assert np.array_equal(z["rgba8"], np.floor(255.0 * z["rgba"] + 0.5).astype(np.uint8))
    assert tuple(pal.entries[0]) == (0, 0, 0, 255) and (pal.entries[:, 3] == 255).all()
    # the fixture does hold ties, which is why the rounding rule is in the contract
    assert (255.0 * z["rgba"] == np.floor(255.0 * z["rgba"]) + 0.5).any()


@pytest.mark.parametrize("s", M.SUPERSAMPLES)
def test_bytes_source_equals_the_model(s):
    rs = np.random.RandomState(100 + s)
    for w, h in [(1, 1), (5, 3), (37, 11), (64, 2)]:
        pal = _random_palette(rs, 256)
        b = rs.randint(0, 256, (h * s, w * s)).astype(np.uint8)
        got = resolve_host(pal, "bytes", s, w, h, bytes_=b)
        assert np.array_equal(got, M.render_bytes(pal.entries, s, b)), (s, w, h)
    # the viewer palette on every byte value
    b = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16), s, axis=0), s, axis=1)
    assert np.array_equal(resolve_host(Palette.viewer(), "bytes", s, 16, 16, bytes_=b),
                          Palette.viewer().entries.reshape(16, 16, 4))


@pytest.mark.parametrize("n", [2, 3, 256, 4097, 65536])
@pytest.mark.parametrize("s", M.SUPERSAMPLES)
def test_smooth_source_equals_the_model_on_random_samples(s, n):
    rs = np.random.RandomState(1000 * s + n % 997)
    w, h = 23, 9
    pal = _random_palette(rs, n)
    shape = (h * s, w * s)
    counts = rs.randint(0, 6, shape).astype(np.int32) * rs.randint(1, 5000, shape).astype(np.int32)   # a sixth are 0
    nu = np.where(rs.rand(*shape) < 0.5, rs.uniform(-3.0, 40.0, shape), rs.uniform(0.0, 3e6, shape))
    got = resolve_host(pal, "smooth", s, w, h, counts=counts, smooth=nu)
    want = M.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, s, counts, nu)
    assert np.array_equal(got, want), int((got != want).sum())


def _one(pal, count, nu):
    """One sample at s = 1 through the library and through the model."""
    c = np.array([[count]], np.int32)
    v = np.array([[nu]], np.float64)
    got = resolve_host(pal, "smooth", 1, 1, 1, counts=c, smooth=v)[0, 0]
    want = M.render_smooth(pal.entries, pal.inside, pal.scale, pal.offset, 1, c, v)[0, 0]
    assert np.array_equal(got, want), (count, nu, got, want)
    return tuple(int(x) for x in got)


def test_smooth_edge_cases_by_name():
    rs = np.random.RandomState(5)
    e = rs.randint(0, 256, (7, 4)).astype(np.uint8)
    pal = Palette(e, inside=(9, 8, 7, 6), scale=1.0, offset=0.0)
    p = lambda k: tuple(int(x) for x in e[k])   # noqa: E731
    # count 0 with a non-zero nu: decided on the count
    assert _one(pal, 0, 3.25) == (9, 8, 7, 6)
    # a count that is not 0 with nu = 0: not `inside`
    assert _one(pal, 4, 0.0) == p(0)
    # nu = -inf (|z|^2 overflowed), NaN, and a negative t: entry 0 exactly
    assert _one(pal, 1, -np.inf) == p(0)
    assert _one(pal, 1, np.nan) == p(0)
    assert _one(Palette(e, scale=2.0, offset=-10.0), 1, 4.5) == p(0)
    # t an exact integer: f = 0, the entry itself
    assert _one(pal, 2, 3.0) == p(3)
    # f = 255: one 256th short of the next entry
    got = _one(pal, 2, 3.0 + 255.0 / 256.0)
    assert got == tuple((int(e[3, c]) * 1 + int(e[4, c]) * 255 + 128) >> 8 for c in range(4))
    # just below the next integer: f is still 255, never 256
    _one(pal, 2, np.nextafter(4.0, 0.0))
    # k = n - 1 wraps to entry 0
    got = _one(pal, 2, 6.5)
    assert got == tuple((int(e[6, c]) * 128 + int(e[0, c]) * 128 + 128) >> 8 for c in range(4))
    assert _one(pal, 2, 7.0) == p(0) and _one(pal, 2, 7.0 * 12345 + 5.0) == p(5)
    # the largest scale with nu near 2^31: t ~ 2^51, still exact (palettes that do and do not divide 2^k)
    for n in (2, 3, 7, 256, 4097, 65535, 65536):
        big = Palette(rs.randint(0, 256, (n, 4)).astype(np.uint8), scale=2.0 ** 20, offset=2.0 ** 20)
        for nu in (2.0 ** 31, 2.0 ** 31 - 1.0 + 2.0 ** -21, np.nextafter(2.0 ** 31, 0.0), 2147483646.999, 2.0 ** 31 + 1.0):
            _one(big, 2 ** 31 - 1, nu)
        small = Palette(big.entries, scale=2.0 ** -30, offset=-(2.0 ** 20))
        _one(small, 5, 2.0 ** 31)


def test_index_arithmetic_near_multiples_of_the_palette_length():
    """k mod n through the quotient estimate: k = q n - 1, q n, q n + 1 for large q and awkward n."""
    rs = np.random.RandomState(6)
    for n in (3, 7, 255, 257, 4097, 65535):
        pal = Palette(rs.randint(0, 256, (n, 4)).astype(np.uint8), scale=1.0, offset=0.0)
        q = rs.randint(1, 2 ** 31, 64).astype(np.int64) * rs.randint(1, 2 ** 20, 64).astype(np.int64) // n
        ks = np.concatenate([q * n - 1, q * n, q * n + 1]).astype(np.float64)
        ks = ks[ks < 2.0 ** 51]
        side = len(ks)
        counts = np.ones((1, side), np.int32)
        got = resolve_host(pal, "smooth", 1, side, 1, counts=counts, smooth=ks[None, :])
        want = M.render_smooth(pal.entries, pal.inside, 1.0, 0.0, 1, counts, ks[None, :])
        assert np.array_equal(got, want), n


def _spec(**kw):
    pal = kw.pop("palette", np.zeros((256, 4), np.uint8))
    d = dict(source=L.MBK_RENDER_BYTES, supersample=1, palette=pal.ctypes.data if pal is not None else None,
             palette_len=0 if pal is None else len(pal), scale=1.0, offset=0.0, max_band_rows=0)
    d.update(kw)
    return L.mbk_render_spec(d["source"], d["supersample"], d["palette"], d["palette_len"], (C.c_uint8 * 4)(0, 0, 0, 255),
                             d["scale"], d["offset"], d["max_band_rows"]), pal


def test_host_call_refuses_bad_arguments_and_writes_nothing():
    lib = L.load()
    w, h = 4, 3
    pal2 = np.zeros((2, 4), np.uint8)
    smooth = dict(source=L.MBK_RENDER_SMOOTH, palette=pal2)
    bad = {
        "unknown source": _spec(source=7),
        "s = 0": _spec(supersample=0), "s = 5": _spec(supersample=5), "s = 16": _spec(supersample=16),
        "NULL palette": _spec(palette=None, palette_len=256),
        "bytes palette of 255": _spec(palette=np.zeros((255, 4), np.uint8)),
        "bytes palette of 257": _spec(palette=np.zeros((257, 4), np.uint8)),
        "smooth palette of 1": _spec(source=L.MBK_RENDER_SMOOTH, palette=np.zeros((1, 4), np.uint8)),
        "smooth palette of 65537": _spec(source=L.MBK_RENDER_SMOOTH, palette=np.zeros((65537, 4), np.uint8)),
        "scale 0": _spec(scale=0.0, **smooth), "scale < 0": _spec(scale=-1.0, **smooth),
        "scale > 2^20": _spec(scale=np.nextafter(2.0 ** 20, np.inf), **smooth),
        "scale inf": _spec(scale=np.inf, **smooth), "scale nan": _spec(scale=np.nan, **smooth),
        "offset > 2^20": _spec(offset=2.0 ** 20 + 1, **smooth), "offset < -2^20": _spec(offset=-(2.0 ** 20) - 1, **smooth),
        "offset inf": _spec(offset=-np.inf, **smooth), "offset nan": _spec(offset=np.nan, **smooth),
    }
    counts = np.ones((h * 8, w * 8), np.int32)
    byts = np.ones((h * 8, w * 8), np.uint8)
    nu = np.ones((h * 8, w * 8), np.float64)

    def call(spec, width=w, height=h, c=counts, b=byts, v=nu, out=True):
        rgba = np.full((h, w, 4), 0xA5, np.uint8)
        st = lib.mbk_render_resolve_host(C.byref(spec) if spec is not None else None, width, height,
                                         c.ctypes.data if c is not None else None, b.ctypes.data if b is not None else None,
                                         v.ctypes.data if v is not None else None, rgba.ctypes.data if out else None)
        assert (rgba == 0xA5).all() or st == L.MBK_OK
        return st

    for name, (spec, _keep) in bad.items():
        assert call(spec) == L.MBK_ERR_INVALID, name
    ok_b, _k1 = _spec()
    ok_s, _k2 = _spec(**smooth)
    assert call(None) == L.MBK_ERR_INVALID
    assert call(ok_b, out=False) == L.MBK_ERR_INVALID
    assert call(ok_b, width=0) == L.MBK_ERR_INVALID and call(ok_b, height=0) == L.MBK_ERR_INVALID
    big, _k3 = _spec(supersample=8)
    assert call(big, width=2 ** 28) == L.MBK_ERR_INVALID
    assert call(ok_b, b=None) == L.MBK_ERR_INVALID
    assert call(ok_s, c=None) == L.MBK_ERR_INVALID and call(ok_s, v=None) == L.MBK_ERR_INVALID
    # ... and the accepted edges of the ranges
    assert call(ok_b) == L.MBK_OK and call(ok_s) == L.MBK_OK
    assert call(ok_b, c=None, v=None) == L.MBK_OK and call(ok_s, b=None) == L.MBK_OK
    for kw in (dict(scale=2.0 ** 20), dict(scale=5e-324), dict(offset=2.0 ** 20), dict(offset=-(2.0 ** 20))):
        assert call(_spec(**kw, **smooth)[0]) == L.MBK_OK, kw
    with pytest.raises(MbkError):
        resolve_host(Palette(np.zeros((5, 4), np.uint8)), "bytes", 1, 2, 2, bytes_=np.zeros((2, 2), np.uint8))


def _read_png(path):
    """8-bit RGBA, non-interlaced, filter type 0 only."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 4)


def test_write_png_round_trips(tmp_path):
    rs = np.random.RandomState(8)
    for shape in [(1, 1, 4), (3, 5, 4), (67, 130, 4)]:
        img = rs.randint(0, 256, shape).astype(np.uint8)
        write_png(tmp_path / "a.png", img, flip=False)
        assert np.array_equal(_read_png(tmp_path / "a.png"), img)
        write_png(tmp_path / "b.png", img)   # row 0 of a render is the lowest imaginary part: the bottom line of the picture
        assert np.array_equal(_read_png(tmp_path / "b.png"), img[::-1])
    for bad in (np.zeros((3, 5, 3), np.uint8), np.zeros((3, 5, 4), np.float32), np.zeros((0, 5, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(tmp_path / "c.png", bad)


def test_palettes_are_well_formed_and_no_imaging_library_is_imported():
    import re
    for pal in (Palette.cosine(), Palette.cosine(300, period=8.0), Palette.gradient([(0, 7, 100), (255, 255, 255), (255, 170, 0)])):
        assert pal.entries.dtype == np.uint8 and pal.entries.shape[1] == 4 and 2 <= len(pal) <= 65536
        assert 0.0 < pal.scale <= 2.0 ** 20 and (pal.entries[:, 3] == 255).all()
    pkg = os.path.join(ROOT, "distributedmandelbrot_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            text = open(os.path.join(pkg, f)).read()
            assert not re.search(r"^\s*(from|import)\s+(PIL|matplotlib|imageio|cv2|skimage)\b", text, flags=re.M), f
