"""Stored chunks on the GPU (include/mbk.h, "Stored chunks"): the device decoder against the independent host decoder and the
original bytes, the device validator's reason codes and bounds, the colour + resolve kernels against tests/chunk_model.py and
the host functions, and viewer.render_level end to end from a store and from a DataServer.  Every comparison is bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import chunk_model as M
from conftest import ROOT
from distributedmandelbrot_amd import MbkError
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import viewer
from distributedmandelbrot_amd.chunkstore import ChunkStore, deserialize_chunk
from distributedmandelbrot_amd.device import decode_chunk_host
from distributedmandelbrot_amd.image import Palette, resolve_chunk_host
from distributedmandelbrot_amd.server import DataServer
from oracle.serializer import serialize
import render_model

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 4096


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_codec_golden", os.path.join(ROOT, "tests", "golden", "make_codec_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pinned(gpu, stream):
    buf = gpu.pinned_empty((len(stream),), np.uint8)
    buf[:] = np.frombuffer(stream, np.uint8)
    return buf


def _expect_stats(st, data):
    assert st.rle_runs == M.maximal_runs(data)
    assert st.all_bytes_zero == (not data.any()) and st.all_bytes_one == bool((data == 1).all())
    assert st.pixel_iterations == 0 and st.never_pixels == 0


def test_decode_every_pattern_through_compute(gpu, gen):
    """6a: decode_chunk == deserialize_chunk == the original bytes, small n included; the statistics of the decoded bytes."""
    for name in gen.PATTERNS:
        data = gen.pattern(name)
        stream = serialize(data)
        got, st = gpu.decode_chunk(stream, data.size)
        assert np.array_equal(got, data), name
        assert np.array_equal(got, deserialize_chunk(stream, data.size)), name
        _expect_stats(st, data)
    for n, runs in ((10, 2), (4099, 501), (M.CHUNK, 5000)):     # non-maximal runs, Raw with trailing bytes, RLE of 1 + n
        for name, stream, decoded in M.unusual_valid_streams(n, runs):
            got, st = gpu.decode_chunk(stream, n)
            assert np.array_equal(got, decoded), (n, name)
            _expect_stats(st, decoded)


def test_decode_inverts_the_device_serialiser_and_leaves_it_alone(gpu):
    """6b: two golden tiles computed and serialised on the device come back as their bytes; mbk_serialize_last still refers
    to the tile, not to the decoded chunk."""
    for level, mrd, ir, ii in ((4, 256, 1, 2), (10, 1024, 3, 5)):
        byts, _, st = gpu.datachunk(level, mrd, ir, ii)
        byts = byts.ravel().copy()
        stream, codec = gpu.serialize_last()
        got, dst = gpu.decode_chunk(stream)
        assert np.array_equal(got, byts) and np.array_equal(deserialize_chunk(stream), byts)
        assert dst.rle_runs == st.rle_runs and (codec == 0 or len(stream) == 1 + 5 * dst.rle_runs)
        gpu.decode_chunk(serialize(np.zeros(M.CHUNK, np.uint8)))
        assert gpu.serialize_last() == (stream, codec)


def test_decode_through_launch_on_a_stream_with_pinned_input(gpu, gen):
    """6c: asynchronous, on a non-default stream; a long stream followed by a short one on the same stream (stale scratch);
    an output address that is not 16-byte aligned; guards intact."""
    import torch
    hip_stream = torch.cuda.Stream()
    order = ["rle_wins_by_a_hair_chunk", "long_runs_chunk", "all_one_chunk", "noisy_chunk", "rle_wins_by_a_hair_chunk", "tie_small"]
    for name, shift in zip(order, (0, 0, 0, 0, 3, 1)):
        data = gen.pattern(name)
        n = data.size
        pinned = _pinned(gpu, serialize(data))
        buf = torch.full((GUARD + shift + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        status = torch.full((1,), 0x7f7f7f7f, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(hip_stream):
            gpu.launch_decode_chunk(pinned, d_bytes=buf.data_ptr() + GUARD + shift, n=n, d_status=status.data_ptr(),
                                    hip_stream=hip_stream.cuda_stream)
        hip_stream.synchronize()
        got = buf.cpu().numpy()
        assert int(status.cpu()[0]) == M.OK, name
        assert np.array_equal(got[GUARD + shift:GUARD + shift + n], data), (name, shift)
        assert (got[:GUARD + shift] == SENTINEL).all() and (got[GUARD + shift + n:] == SENTINEL).all(), (name, shift)


@pytest.mark.parametrize("n,runs", [(64, 3), (1000, 100), (M.CHUNK, 5000)])
def test_invalid_streams_through_compute(gpu, n, runs):
    """7a: the error, the reason in its message, the host buffer untouched.  Malformed inputs, checked by clamped code."""
    for name, stream, reason in M.invalid_streams(n, runs):
        out = np.full(n, SENTINEL, np.uint8)
        with pytest.raises(MbkError) as e:
            gpu.decode_chunk(stream, n, out)
        assert e.value.status == L.MBK_ERR_INVALID and M.REASON_NAMES[reason] in str(e.value), (name, str(e.value))
        assert (out == SENTINEL).all(), name
    good = M.unusual_valid_streams(n, runs)[0]
    assert np.array_equal(gpu.decode_chunk(good[1], n)[0], good[2])      # and the ctx carries on


@pytest.mark.parametrize("n,runs", [(1000, 100), (M.CHUNK, 5000)])
def test_invalid_streams_through_launch_keep_their_bounds(gpu, n, runs):
    """7b: into a device buffer with guard bytes before and after: what the host sees without walking the payload is refused
    at once; everything else is judged on the device: status word = the reason, guards intact."""
    import torch
    on_device = 0
    for name, stream, reason in M.invalid_streams(n, runs):
        buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        status = torch.full((1,), 0x7f7f7f7f, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        try:
            gpu.launch_decode_chunk(stream, d_bytes=buf.data_ptr() + GUARD, n=n, d_status=status.data_ptr())
        except MbkError as e:
            assert M.REASON_NAMES[reason] in str(e), name
            assert reason in (M.BAD_CODEC, M.BAD_SIZE) or len(stream) <= 6, name     # only what needs no walk
            torch.cuda.synchronize()
            assert int(status.cpu()[0]) == 0x7f7f7f7f and (buf.cpu().numpy() == SENTINEL).all(), name
            continue
        torch.cuda.synchronize()
        on_device += 1
        assert int(status.cpu()[0]) == reason, (name, int(status.cpu()[0]))
        got = buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n:] == SENTINEL).all(), name
    assert on_device >= 8


def _render_streams(gpu, gen):
    byts, _, _ = gpu.datachunk(4, 256, 1, 1)
    out = {"tile_4_256_1_1": (serialize(byts.ravel()), byts.ravel().copy())}
    for name in ("long_runs_chunk", "noisy_chunk"):
        out[name] = (serialize(gen.pattern(name)), gen.pattern(name))
    zero = gen.pattern("all_zero_chunk")
    out["all_zero_one_run"] = (serialize(zero), zero)
    out["all_zero_two_runs"] = (M.rle_stream([M.CHUNK - 12345, 12345], [0, 0]), zero)      # the long way round
    return out


def test_render_equals_the_model_and_the_host_functions(gpu, gen):
    """8a: every k x {random palette, the Viewer's} x {a boundary tile, long runs, Raw, one value as one run and as two}."""
    streams = _render_streams(gpu, gen)
    assert len(streams["all_zero_one_run"][0]) == 6 and len(streams["all_zero_two_runs"][0]) == 11
    for pname, pal in (("random", Palette(M.random_palette())), ("viewer", Palette.viewer())):
        for k in M.SCALES:
            images = {}
            for name, (stream, byts) in streams.items():
                got, st = gpu.render_chunk(stream, palette=pal, scale=k)
                images[name] = got
                if name == "all_zero_two_runs":
                    assert np.array_equal(got, images["all_zero_one_run"]), (pname, k)
                    continue
                assert np.array_equal(got, M.resolve(pal.entries, k, byts)), (pname, k, name)
                assert st.rle_runs == 0 and st.pixel_iterations == 0
            assert (images["all_zero_one_run"] == pal.entries[0]).all()
    pal = Palette(M.random_palette())
    _, byts = streams["tile_4_256_1_1"]
    for k in M.SCALES:      # ... and the host functions of the decoded bytes
        got, _ = gpu.render_chunk(streams["tile_4_256_1_1"][0], palette=pal, scale=k)
        assert np.array_equal(got, resolve_chunk_host(pal, k, decode_chunk_host(streams["tile_4_256_1_1"][0]))), k
        if k <= 8:          # the rule of the view renders, which tests/test_gpu_render.py ties to mbk_view_render_*
            assert np.array_equal(got, render_model.render_bytes(pal.entries, k, byts.reshape(M.DIM, M.DIM))), k


def test_render_with_a_pitch_into_larger_images(gpu, gen):
    """8b: into a larger host image (compute) and a larger device image with guards (launch, every k, both shortcut and long
    way): the rectangle is the chunk, everything else keeps the sentinel."""
    import torch
    streams = _render_streams(gpu, gen)
    pal = Palette(M.random_palette())
    hip_stream = torch.cuda.Stream()
    pinned = {name: _pinned(gpu, streams[name][0]) for name in ("long_runs_chunk", "all_zero_one_run", "noisy_chunk")}
    for k in M.SCALES:
        w = M.DIM // k
        pitch, rows, x0, y0 = w + 24 + (k == 4), w + 3, 7 if k != 2 else 8, 2
        for name in ("long_runs_chunk", "all_zero_one_run", "noisy_chunk"):
            stream, byts = streams[name]
            want = np.full((rows, pitch, 4), SENTINEL, np.uint8)
            want[y0:y0 + w, x0:x0 + w] = M.resolve(pal.entries, k, byts)
            host = np.full((rows, pitch, 4), SENTINEL, np.uint8)
            gpu.render_chunk(stream, palette=pal, scale=k, out=host[y0:, x0:], pitch=pitch)
            assert np.array_equal(host, want), (k, name, "compute")
            buf = torch.full((GUARD + rows * pitch * 4 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
            status = torch.full((1,), 0x7f7f7f7f, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(hip_stream):
                gpu.launch_render_chunk(pinned[name], d_rgba=buf.data_ptr() + GUARD + 4 * (y0 * pitch + x0), palette=pal,
                                        scale=k, pitch=pitch, d_status=status.data_ptr(), hip_stream=hip_stream.cuda_stream)
            hip_stream.synchronize()
            got = buf.cpu().numpy()
            assert int(status.cpu()[0]) == M.OK
            assert np.array_equal(got[GUARD:-GUARD].reshape(rows, pitch, 4), want), (k, name, "launch")
            assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), (k, name)


def test_invalid_streams_through_render(gpu):
    """7c: the render forms refuse what the decoder refuses: host image untouched, device image inside its bounds."""
    import torch
    pal = Palette.viewer()
    k, w = 16, 256
    for name, stream, reason in M.invalid_streams(M.CHUNK, 5000):
        host = np.full((w, w, 4), SENTINEL, np.uint8)
        with pytest.raises(MbkError) as e:
            gpu.render_chunk(stream, palette=pal, scale=k, out=host)
        assert M.REASON_NAMES[reason] in str(e.value) and (host == SENTINEL).all(), name
    name, stream, reason = M.invalid_streams(M.CHUNK, 5000)[4]
    assert name == "sum_n_plus_1"
    buf = torch.full((GUARD + w * w * 4 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    status = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_chunk(stream, d_rgba=buf.data_ptr() + GUARD, palette=pal, scale=k, d_status=status.data_ptr())
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert int(status.cpu()[0]) == reason and (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all()
    for bad in ({"scale": 3}, {"scale": 128}, {"scale": 16, "pitch": 255, "out": np.empty((256, 255, 4), np.uint8)}):
        with pytest.raises(MbkError):
            gpu.render_chunk(M.rle_stream([M.CHUNK], [1]), palette=pal, **bad)


def test_render_level_end_to_end_from_a_store_and_a_server(gpu, oracle, tmp_path):
    """9: four tiles of level 2 computed and stored from the device, then the level as one image at k = 8, from the store and
    from a DataServer: identical, and equal to the model applied to the ORACLE's tiles mosaicked by hand."""
    store = ChunkStore(str(tmp_path))
    tiles = {}
    for ir in range(2):
        for ii in range(2):
            store.save_from_device(gpu, 2, 256, ir, ii)
            tiles[(ir, ii)] = oracle.datachunk(2, 256, ir, ii, want_counts=False)[1].ravel()
    pal = Palette.viewer()
    img, missing = viewer.render_level(gpu, store, 2, scale=8)
    assert missing == [] and img.shape == (1024, 1024, 4)
    want = M.mosaic(pal.entries, 8, tiles, 0, 0, 2, 2)
    assert np.array_equal(img, want)
    with DataServer(store) as ds:
        img2, missing2 = viewer.render_level(gpu, ("127.0.0.1", ds.port), 2, scale=8)
    assert missing2 == [] and np.array_equal(img2, img)
    by_hand = np.empty_like(want)
    for (ir, ii), b in tiles.items():
        by_hand[ii * 512:(ii + 1) * 512, ir * 512:(ir + 1) * 512] = render_model.render_bytes(pal.entries, 8, b.reshape(M.DIM, M.DIM))
    assert np.array_equal(img, by_hand)
    for k in (1, 2, 4):     # the chunk render of a tile == the view renders' rule on the tile's bytes
        stream = store.load_serialized(store.find(2, 1, 0))
        got, _ = gpu.render_chunk(stream, palette=pal, scale=k)
        assert np.array_equal(got, render_model.render_bytes(pal.entries, k, tiles[(1, 0)].reshape(M.DIM, M.DIM))), k
    part, missing3 = viewer.render_level(gpu, store, 3, region=(0, 0, 1, 1), scale=64, missing=(9, 9, 9, 9))
    assert missing3 == [(0, 0)] and (part == 9).all()
