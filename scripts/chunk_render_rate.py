#!/usr/bin/env python3
"""Stored-chunk measurements (profiles/chunks/README.md).

    python scripts/chunk_render_rate.py chunks    per chunk: decode_chunk and render_chunk (k = 1, 8, 64) for (a) one run,
                                                  (b) a boundary tile, (c) 3.3 M runs of five, (d) a Raw chunk -- kernel time
                                                  (HIP events, TileStats.kernel_ms) and wall time; beside each the host path
                                                  (deserialize_chunk + resolve_host, k <= 8) and the H2D copy of the stream alone
    python scripts/chunk_render_rate.py level16   render_level of a whole level-16 store at k = 16: wall time, chunks / s
    python scripts/chunk_render_rate.py kernels   a few decodes and renders of every kind -- run under
                                                  `rocprofv3 --kernel-trace --stats -- python scripts/chunk_render_rate.py kernels`
                                                  for each kernel's own time

Legs alternate within one process and each lasts >= 50 ms after a warm-up, as bench.py does it.  Streams and images live in
pinned memory."""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedmandelbrot_amd import MandelbrotDevice, Palette   # noqa: E402
from distributedmandelbrot_amd import viewer   # noqa: E402
from distributedmandelbrot_amd.chunkstore import CHUNK_BYTES, ChunkStore, deserialize_chunk, serialize_chunk   # noqa: E402
from distributedmandelbrot_amd.image import resolve_host   # noqa: E402

SCALES = (1, 8, 64)


def leg(fn, min_seconds=0.05, min_calls=3):
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and n >= min_calls:
            return dt / n


def streams(dev):
    v = (np.arange(CHUNK_BYTES // 5 + 1) % 251).astype(np.uint8)
    v[1], v[3] = v[0], v[2]                                     # RLE wins by a hair: 3 355 442 runs
    tile, _, _ = dev.datachunk(4, 256, 1, 1)
    tile_stream, _ = dev.serialize_last()
    out = {"a_one_run": bytes([1]) + (CHUNK_BYTES).to_bytes(4, "little") + b"\x00",
           "b_boundary_tile_4_256_1_1": tile_stream,
           "c_runs_of_five": serialize_chunk(np.repeat(v, 5)[:CHUNK_BYTES]),
           "d_raw": serialize_chunk(np.random.RandomState(1).randint(0, 256, CHUNK_BYTES, dtype=np.uint8))}
    pinned = {}
    for name, s in out.items():
        pinned[name] = dev.pinned_empty((len(s),), np.uint8)
        pinned[name][:] = np.frombuffer(s, np.uint8)
    return out, pinned


def h2d_alone(pinned_stream, seconds=0.05):
    """The stream's upload by itself (pinned host -> device), timed with device events."""
    import torch
    src = torch.from_numpy(np.asarray(pinned_stream))          # the library's pinned memory: the copy is a plain DMA
    dst = torch.empty(src.numel(), dtype=torch.uint8, device="cuda:0")
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    reps = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    while True:
        for _ in range(8):
            dst.copy_(src, non_blocking=True)
        reps += 8
        if time.perf_counter() - t0 >= seconds:
            break
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def chunks():
    pal = Palette.viewer()
    with MandelbrotDevice(0) as dev:
        plain, pinned = streams(dev)
        out_bytes = dev.pinned_empty((CHUNK_BYTES,), np.uint8)
        images = {k: dev.pinned_empty((4096 // k, 4096 // k, 4), np.uint8) for k in SCALES}
        for _ in range(20):                                      # clock ramp
            dev.render_chunk(pinned["c_runs_of_five"], palette=pal, scale=1, out=images[1])
        legs = {}
        for name in plain:
            legs[(name, "decode")] = lambda name=name: dev.decode_chunk(pinned[name], out=out_bytes)
            for k in SCALES:
                legs[(name, f"render_k{k}")] = lambda name=name, k=k: dev.render_chunk(pinned[name], palette=pal, scale=k, out=images[k])
        rounds = {key: [] for key in legs}
        kernel = {key: [] for key in legs}
        for _ in range(3):
            for key, fn in legs.items():
                rounds[key].append(leg(fn) * 1e3)
                kernel[key].append(fn()[1].kernel_ms)
        result = {"device": dev.info()["name"], "pci": dev.pci_bus_id(), "streams": {}}
        for name, s in plain.items():
            row = {"stream_bytes": len(s), "h2d_alone_ms": h2d_alone(pinned[name])}
            for (nm, what), v in rounds.items():
                if nm == name:
                    row[what] = {"wall_ms": float(np.median(v)), "wall_min_ms": min(v), "wall_max_ms": max(v),
                                 "kernel_ms": float(np.median(kernel[(nm, what)]))}
            # the host path of the parent commit for the same job (numpy decode; the C resolve of the view renders, s <= 8)
            t0 = time.perf_counter()
            byts = deserialize_chunk(s)
            row["host_deserialize_chunk_ms"] = (time.perf_counter() - t0) * 1e3
            for k in (1, 8):
                t0 = time.perf_counter()
                resolve_host(pal, "bytes", k, 4096 // k, 4096 // k, bytes_=byts)
                row[f"host_resolve_host_k{k}_ms"] = (time.perf_counter() - t0) * 1e3
            result["streams"][name] = row
        print(json.dumps(result))


def level16():
    with MandelbrotDevice(0) as dev, tempfile.TemporaryDirectory() as tmp:
        store = ChunkStore(tmp)
        t0 = time.perf_counter()
        for ir in range(16):
            for ii in range(16):
                store.save_from_device(dev, 16, 1024, ir, ii)
        fill = time.perf_counter() - t0
        types = [e.type for e in store.entries()]
        img = dev.pinned_empty((4096, 4096, 4), np.uint8)
        viewer.render_level(dev, store, 16, scale=16, out=img)  # warm-up: scratch, palette, file cache
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            viewer.render_level(dev, store, 16, scale=16, out=img)
            walls.append(time.perf_counter() - t0)
        w = float(np.median(walls))
        print(json.dumps({"device": dev.info()["name"], "pci": dev.pci_bus_id(), "store_fill_s": fill,
                          "regular": types.count(0), "never": types.count(1), "immediate": types.count(2),
                          "file_bytes": sum(os.path.getsize(os.path.join(store.data_dir, e.filename)) for e in store.entries() if e.type == 0),
                          "render_level_k16_wall_s": w, "wall_min_s": min(walls), "wall_max_s": max(walls),
                          "chunks_per_s": 256 / w, "regular_chunks_per_s": types.count(0) / w}))


def kernels():
    pal = Palette.viewer()
    with MandelbrotDevice(0) as dev:
        _, pinned = streams(dev)
        out_bytes = dev.pinned_empty((CHUNK_BYTES,), np.uint8)
        img = dev.pinned_empty((4096, 4096, 4), np.uint8)
        for name in pinned:
            for _ in range(6):
                dev.decode_chunk(pinned[name], out=out_bytes)
            for k in (1, 2, 4, 8, 16, 32, 64):
                for _ in range(6):
                    dev.render_chunk(pinned[name], palette=pal, scale=k, out=img.reshape(-1)[:(4096 // k) ** 2 * 4].reshape(4096 // k, 4096 // k, 4))
        print("done", dev.info()["name"], dev.pci_bus_id())


if __name__ == "__main__":
    {"chunks": chunks, "level16": level16, "kernels": kernels}[sys.argv[1]]()
