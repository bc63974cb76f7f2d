"""Stored chunks on the host (include/mbk.h, "Stored chunks"): the stream rules, the decoder and the colour + resolve rule of
mbk_chunk_*_host -- the functions the kernels are compiled from -- against tests/chunk_model.py, the reference decoder's
recorded output (tests/golden/codec_vectors.npz) and the reference Viewer's recorded colours (viewer_palette.npz); and
viewer.py (the DataServer exchange, the mosaic, the command line) with a device that runs the host functions.  No GPU."""
import hashlib
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import chunk_model as M
from conftest import ROOT
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import viewer
from distributedmandelbrot_amd.chunkstore import ChunkStore, deserialize_chunk
from distributedmandelbrot_amd.device import ChunkStreamError, MbkError, TileStats, chunk_stream_check, decode_chunk_host
from distributedmandelbrot_amd.image import Palette, resolve_chunk_host
from distributedmandelbrot_amd.server import DataServer
from oracle.serializer import serialize

SENTINEL = 0xA5


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def codec_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_vectors.npz"))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_codec_golden", os.path.join(ROOT, "tests", "golden", "make_codec_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def boundary_tile(oracle):
    return oracle.datachunk(4, 256, 1, 2, want_counts=False)[1].ravel()


def test_reason_codes_and_scales_match_the_model():
    assert [L.STREAM_REASONS[k] for k in range(6)] == M.REASON_NAMES
    assert L.CHUNK_SCALES == M.SCALES and L.MBK_CHUNK_BYTES == M.CHUNK


def test_every_pattern_decodes_to_what_the_reference_decoder_returned(codec_golden, gen):
    """1: check and decode of the pinned streams: codec, length, and the hash the REFERENCE's decoder produced."""
    assert list(gen.PATTERNS) == [str(n) for n in codec_golden["pattern/names"]]
    for name in gen.PATTERNS:
        data = gen.pattern(name)
        stream = serialize(data)
        assert sha(stream) == str(codec_golden[f"pattern/{name}/stream_sha256"]), name
        codec, runs = chunk_stream_check(stream, data.size)
        assert codec == int(codec_golden[f"pattern/{name}/codec"]) == stream[0], name
        assert len(stream) == int(codec_golden[f"pattern/{name}/stream_len"]) == (1 + 5 * runs if codec else 1 + data.size), name
        assert (codec, runs) == M.check(stream, data.size)[:2]
        got = decode_chunk_host(stream, data.size)
        assert sha(got) == str(codec_golden[f"pattern/{name}/decoded_sha256"]), name
        assert np.array_equal(got, M.decode(stream, data.size))


@pytest.mark.parametrize("n,runs", [(64, 3), (1000, 100), (M.CHUNK, 5000)])
def test_invalid_streams_are_refused_with_the_documented_reason(n, runs):
    """2: one stream per reason code and boundary: MBK_ERR_INVALID, the reason, the output untouched -- and the independent
    decoder (chunkstore.deserialize_chunk) refuses every one of them too."""
    for name, stream, reason in M.invalid_streams(n, runs):
        with pytest.raises(M.StreamInvalid) as m:
            M.check(stream, n)
        assert m.value.reason == reason, name
        with pytest.raises(ChunkStreamError) as e:
            chunk_stream_check(stream, n)
        assert e.value.reason == reason and e.value.status == L.MBK_ERR_INVALID, (name, e.value.reason)
        assert M.REASON_NAMES[reason] in str(e.value), name
        out = np.full(n, SENTINEL, np.uint8)
        with pytest.raises(MbkError) as e:
            decode_chunk_host(stream, n, out)
        assert e.value.status == L.MBK_ERR_INVALID and M.REASON_NAMES[reason] in str(e.value), name
        assert (out == SENTINEL).all(), name
        with pytest.raises((ValueError, IndexError)):
            deserialize_chunk(stream, n)


def test_n_outside_the_chunk_is_refused():
    for n in (0, M.CHUNK + 1):
        with pytest.raises(ChunkStreamError) as e:
            chunk_stream_check(bytes([0]) + bytes(8), n)
        assert e.value.reason == M.BAD_SIZE


def test_the_oversized_rle_stream_is_the_one_documented_exception():
    stream, n, decoded = M.oversized_rle_stream()
    assert np.array_equal(deserialize_chunk(stream, n), decoded)      # the independent decoder takes it
    with pytest.raises(ChunkStreamError) as e:
        chunk_stream_check(stream, n)
    assert e.value.reason == M.BAD_SIZE
    out = np.full(n, SENTINEL, np.uint8)
    with pytest.raises(MbkError):
        decode_chunk_host(stream, n, out)
    assert (out == SENTINEL).all()
    with pytest.raises(M.StreamInvalid) as m:
        M.check(stream, n)
    assert m.value.reason == M.BAD_SIZE


@pytest.mark.parametrize("n,runs", [(10, 2), (64, 3), (4099, 501), (M.CHUNK, 5000)])
def test_valid_but_unusual_streams_decode(n, runs):
    cases = M.unusual_valid_streams(n, runs)
    assert n != 10 or any(len(s) == 1 + n and s[0] == 1 for _, s, _ in cases)
    for name, stream, decoded in cases:
        codec, r = chunk_stream_check(stream, n)
        assert (codec, r) == M.check(stream, n)[:2], name
        got = decode_chunk_host(stream, n)
        assert np.array_equal(got, decoded) and np.array_equal(got, M.decode(stream, n)), name
        assert np.array_equal(deserialize_chunk(stream, n), decoded), name


def _palettes():
    return {"random": Palette(M.random_palette()), "viewer": Palette.viewer()}


@pytest.mark.parametrize("k", M.SCALES)
def test_resolve_host_equals_the_model(k, boundary_tile):
    """3: every k x {random chunk, a golden tile's bytes, a chunk on .5 ties} x {random palette, the Viewer's}."""
    tie_bytes, tie_pal = M.tie_chunk_and_palette()
    chunks = {"random": M.every_value_chunk(), "tile_4_256_1_2": boundary_tile, "ties": tie_bytes}
    for pname, pal in list(_palettes().items()) + [("tie", Palette(tie_pal))]:
        for cname, byts in chunks.items():
            want = M.resolve(pal.entries, k, byts)
            got = resolve_chunk_host(pal, k, byts)
            assert got.shape == want.shape and np.array_equal(got, want), (k, pname, cname)
    if k >= 2:      # the tie chunk does sit on ties: every mean is x.5 and rounds up
        got = resolve_chunk_host(Palette(tie_pal), k, tie_bytes)
        lo = tie_pal[tie_bytes.reshape(M.DIM, M.DIM)[::k, ::k] & 0xfe]
        assert np.array_equal(got, lo + 1)


def test_resolve_host_respects_the_pitch():
    pal = Palette(M.random_palette())
    byts = M.every_value_chunk()
    for k in (4, 64):
        w = M.DIM // k
        pitch = w + 37
        img = np.full((w + 2, pitch, 4), SENTINEL, np.uint8)
        resolve_chunk_host(pal, k, byts, out=img[1:, 5:], pitch=pitch)
        want = np.full_like(img, SENTINEL)
        want[1:w + 1, 5:5 + w] = M.resolve(pal.entries, k, byts)
        assert np.array_equal(img, want), k
    with pytest.raises(MbkError):
        resolve_chunk_host(pal, 4, byts, out=np.empty((1024, 1024, 4), np.uint8), pitch=1023)
    for bad in (0, 3, 128):
        with pytest.raises(MbkError):
            resolve_chunk_host(pal, bad, byts)


@pytest.mark.parametrize("k", M.SCALES)
def test_a_uniform_chunk_renders_as_its_palette_entry(k):
    for pal in _palettes().values():
        for v in (0, 1, 200):
            got = resolve_chunk_host(pal, k, np.full(M.CHUNK, v, np.uint8))
            assert (got == pal.entries[v]).all(), (k, v)


def test_scale_1_with_the_viewer_palette_is_the_reference_viewers_image():
    """4: the reference Viewer's data_to_img_array, 8-bit, as recorded in viewer_palette.npz."""
    rgba8 = np.load(os.path.join(ROOT, "tests", "golden", "viewer_palette.npz"))["rgba8"]
    byts = M.every_value_chunk()
    assert len(np.unique(byts)) == 256
    got = resolve_chunk_host(Palette.viewer(), 1, byts)
    assert np.array_equal(got, rgba8[byts.reshape(M.DIM, M.DIM)])


# ---- viewer.py -------------------------------------------------------------------------------------------------------------

class HostDevice:
    """render_chunk over the host functions: what viewer.render_level needs of a device."""

    def __init__(self):
        self.calls = 0

    def render_chunk(self, stream, *, palette=None, scale=1, out=None, pitch=None):
        self.calls += 1
        byts = decode_chunk_host(stream)
        return resolve_chunk_host(palette, scale, byts, out=out, pitch=pitch), TileStats(0.0, 0.0, 0, 0, False, False)


def test_fetch_chunk_stream_speaks_the_dataserver_protocol(tmp_path, gen):
    """5a: Regular (RLE and Raw files), Never, Immediate, not available, rejected: the bytes are load_serialized's."""
    store = ChunkStore(str(tmp_path))
    placed = {(1, 2): "long_runs_chunk", (0, 0): "all_zero_chunk", (4, 4): "all_one_chunk", (3, 3): "noisy_chunk"}
    for (ir, ii), name in placed.items():
        store.save_chunk(5, ir, ii, gen.pattern(name))
    with DataServer(store) as ds:
        for (ir, ii), name in placed.items():
            got = viewer.fetch_chunk_stream("127.0.0.1", ds.port, 5, ir, ii)
            assert isinstance(got, bytes) and got == store.load_serialized(store.find(5, ir, ii)), name
            assert np.array_equal(decode_chunk_host(got), gen.pattern(name)), name
        assert viewer.fetch_chunk_stream("127.0.0.1", ds.port, 5, 2, 2) is None
        with pytest.raises(ValueError, match="rejected"):
            viewer.fetch_chunk_stream("127.0.0.1", ds.port, 5, 5, 0)


def _level3_store(tmp_path, gen):
    """Level 3 with (2, 1) missing, a Never and an Immediate chunk, RLE and Raw files."""
    rs = np.random.RandomState(31)
    chunks = {}
    for ir in range(3):
        for ii in range(3):
            base = np.repeat(rs.randint(0, 256, M.CHUNK // 2048).astype(np.uint8), 2048)      # long runs: an RLE file
            base[(ii * 3 + ir) * 4096:(ii * 3 + ir) * 4096 + 64] = 255                           # no two chunks alike
            chunks[(ir, ii)] = base
    chunks[(0, 0)] = gen.pattern("all_zero_chunk")
    chunks[(2, 2)] = gen.pattern("all_one_chunk")
    chunks[(1, 1)] = gen.pattern("noisy_chunk")
    chunks[(2, 1)] = None
    store = ChunkStore(str(tmp_path))
    for (ir, ii), b in chunks.items():
        if b is not None:
            store.save_chunk(3, ir, ii, b)
    store.save_chunk(2, 0, 0, gen.pattern("noisy_chunk"))      # another level in the same index
    return store, chunks


def _read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    off, idat, shape = 8, b"", None
    while off < len(raw):
        (n,), tag = struct.unpack(">I", raw[off:off + 4]), raw[off + 4:off + 8]
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", raw[off + 8:off + 18])
            assert (depth, ctype) == (8, 6)
            shape = (h, w)
        if tag == b"IDAT":
            idat += raw[off + 8:off + 8 + n]
        off += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 4 * shape[1])
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(shape[0], shape[1], 4)


def test_render_level_places_every_chunk(tmp_path, gen):
    """5b: placement, orientation, `missing`, host-filled index-only chunks, region cropping, store and server alike."""
    store, chunks = _level3_store(tmp_path, gen)
    pal = Palette(M.random_palette())
    k, miss = 32, (1, 2, 3, 4)
    dev = HostDevice()
    img, missing = viewer.render_level(dev, store, 3, scale=k, palette=pal, missing=miss)
    want = M.mosaic(pal.entries, k, chunks, 0, 0, 3, 3, miss)
    assert img.shape == want.shape == (384, 384, 4) and np.array_equal(img, want)
    assert missing == [(2, 1)]
    assert dev.calls == 6           # 9 chunks: one missing, a Never and an Immediate one filled on the host
    w = M.DIM // k                  # orientation: chunk (ir, ii) at column ir w, row ii w
    assert (img[0:w, 0:w] == pal.entries[0]).all() and (img[2 * w:, 2 * w:] == pal.entries[1]).all()
    assert (img[w:2 * w, 2 * w:] == np.array(miss, np.uint8)).all()

    region = (1, 0, 2, 3)
    out = np.empty((3 * w, 2 * w, 4), np.uint8)
    img2, missing2 = viewer.render_level(dev, store, 3, region=region, scale=k, palette=pal, missing=miss, out=out)
    assert img2 is out and np.array_equal(img2, want[:, w:]) and missing2 == [(2, 1)]
    assert np.array_equal(img2, M.mosaic(pal.entries, k, chunks, *region, missing=miss))

    with DataServer(store) as ds:   # a server sends index-only chunks as one-run streams: all eight go to the device
        dev2 = HostDevice()
        img3, missing3 = viewer.render_level(dev2, ("127.0.0.1", ds.port), 3, scale=k, palette=pal, missing=miss)
        assert np.array_equal(img3, want) and missing3 == [(2, 1)] and dev2.calls == 8

    default_pal, _ = viewer.render_level(HostDevice(), store, 3, region=(0, 0, 1, 1), scale=64)
    assert (default_pal == Palette.viewer().entries[0]).all()
    for bad in ({"region": (0, 0, 4, 1)}, {"region": (3, 0, 1, 1)}, {"scale": 3}, {"region": (0, 0, 0, 1)}):
        with pytest.raises(ValueError):
            viewer.render_level(dev, store, 3, **{"scale": k, **bad})
    with pytest.raises(ValueError, match="2\\^31"):
        viewer.render_level(dev, store, 64, scale=4)       # 65536^2 pixels
    with pytest.raises(ValueError):
        viewer.render_level(dev, store, 0)


def test_the_command_line_writes_the_image_render_level_returns(tmp_path, gen):
    """5c: the PNG's pixels, flipped as write_png documents, are render_level's."""
    store, chunks = _level3_store(tmp_path, gen)
    png = str(tmp_path / "level3.png")
    assert viewer.main(["--store", str(tmp_path), "--level", "3", "--region", "0,1,2,2", "--scale", "64", "--palette", "cosine",
                        png], dev=HostDevice()) == 0
    pal = Palette(Palette.cosine(256).entries)
    want, _ = viewer.render_level(HostDevice(), store, 3, region=(0, 1, 2, 2), scale=64, palette=pal)
    assert np.array_equal(_read_png(png)[::-1], want)
    assert np.array_equal(want, M.mosaic(pal.entries, 64, chunks, 0, 1, 2, 2))
