"""The reference Viewer's job (DistributedMandelbrotViewer.py) on the GPU: fetch stored chunks, from a ChunkStore on disk
or from a DataServer, and turn them into pictures -- one chunk, or a downsampled mosaic of a whole pyramid level, which the
reference cannot show at all (it decodes one chunk in a Python loop and hands 16 Mi pixels to matplotlib).

    python -m distributedmandelbrot_amd.viewer (--store DIR | --server ADDR:PORT) --level L
           [--region IR0,II0,NR,NI] [--scale K] [--palette viewer|cosine] OUT.png

The chunks are decoded, coloured and box-filtered by MandelbrotDevice.render_chunk (include/mbk.h, "Stored chunks"); only the
serialised stream goes up and only the chunk's (4096 / K)^2 pixels come back, straight into their place in the image.
"""
from __future__ import annotations

import argparse
import socket
import struct
import sys
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib as L
from .chunkstore import TYPE_IMMEDIATE, TYPE_NEVER, ChunkStore
from .image import Palette, write_png

MAX_IMAGE_BYTES = 1 << 31


def _recv_exact(s: socket.socket, n: int) -> bytes:
    buf = bytearray(n)
    view, got = memoryview(buf), 0
    while got < n:
        k = s.recv_into(view[got:], n - got)
        if k == 0:
            raise ConnectionError(f"the DataServer closed after {got} of {n} bytes")
        got += k
    return bytes(buf)


def fetch_chunk_stream(addr: str, port: int, level: int, index_real: int, index_imag: int, *,
                       timeout: Optional[float] = 30.0) -> Optional[bytes]:
    """One exchange with a DataServer (DataServer.cs:156-224, as the reference's get_chunk speaks it, Viewer.py:62-108):
    request 3 x u32 (level, indexReal, indexImag); reply status 0x00 + u32 length + the chunk as DataChunk.Serialize wrote
    it -> the stream, UNDECODED; 0x02 (not available) -> None; 0x01 (rejected: an index >= level) -> ValueError."""
    with socket.create_connection((addr, port), timeout=timeout) as s:
        s.sendall(struct.pack("<III", level, index_real, index_imag))
        status = _recv_exact(s, 1)[0]
        if status == 0x02:
            return None
        if status == 0x01:
            raise ValueError(f"the DataServer rejected the request for chunk ({level}; {index_real}, {index_imag})")
        if status != 0x00:
            raise ConnectionError(f"the DataServer answered with unknown status {status:#x}")
        (n,) = struct.unpack("<I", _recv_exact(s, 4))
        return _recv_exact(s, n)


Source = Union[ChunkStore, Tuple[str, int]]


def render_level(dev, source: Source, level: int, *, region: Optional[Sequence[int]] = None, scale: int = 16,
                 palette: Optional[Palette] = None, missing=(0, 0, 0, 0), out: Optional[np.ndarray] = None):
    """A mosaic of the chunks of `level` (any integer >= 1), each at 4096 / scale pixels a side.

    `source` is a ChunkStore or an (addr, port) pair of a DataServer.  `region` = (ir0, ii0, nr, ni) selects whole chunks
    (default: the whole level).  Chunk (ir, ii) lands at columns (ir - ir0) * 4096 / scale and rows (ii - ii0) * 4096 / scale
    of an image whose row 0 is the LOWEST imaginary part (write_png flips it).  Both end points of a tile are sampled, so
    neighbouring chunks share their edge sample: the chunks are simply abutted, and the edge line appears in both.

    Regular chunks go through dev.render_chunk straight into their rectangle of the image (pinned when the device can
    allocate it); the index-only Never / Immediate chunks of a store are filled on the host with palette[0] / palette[1]
    without touching the GPU; chunks the source does not have are filled with `missing` and listed.  A store's index is
    scanned once per call.  Returns (uint8[ni * w, nr * w, 4], [(ir, ii), ...] of the missing chunks)."""
    palette = Palette.viewer() if palette is None else palette
    if scale not in L.CHUNK_SCALES:
        raise ValueError(f"scale must be one of {L.CHUNK_SCALES}")
    if level < 1:
        raise ValueError("level must be >= 1")
    ir0, ii0, nr, ni = (0, 0, level, level) if region is None else (int(v) for v in region)
    if nr < 1 or ni < 1 or ir0 < 0 or ii0 < 0 or ir0 + nr > level or ii0 + ni > level:
        raise ValueError("region = (ir0, ii0, nr, ni) must select whole chunks inside the level")
    w = L.MBK_CHUNK_DEFINITION // scale
    height, width = ni * w, nr * w
    if height * width * 4 > MAX_IMAGE_BYTES:
        raise ValueError(f"a {width} x {height} image exceeds 2^31 bytes: raise scale or narrow the region")
    if out is None:
        alloc = getattr(dev, "pinned_empty", None)
        out = alloc((height, width, 4), np.uint8) if alloc else np.empty((height, width, 4), np.uint8)
    if out.dtype != np.uint8 or out.shape != (height, width, 4) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a contiguous uint8 array of shape {(height, width, 4)}")

    entries = None
    if isinstance(source, ChunkStore):      # one scan of the index; the FIRST entry of a chunk counts, as for ChunkStore.find
        entries = {}
        for e in source.entries():
            if e.level == level:
                entries.setdefault((e.index_real, e.index_imag), e)
    else:
        addr, port = source

    missing_chunks: List[Tuple[int, int]] = []
    for ii in range(ii0, ii0 + ni):
        for ir in range(ir0, ir0 + nr):
            rect = out[(ii - ii0) * w:(ii - ii0 + 1) * w, (ir - ir0) * w:(ir - ir0 + 1) * w]
            stream = None
            if entries is not None:
                e = entries.get((ir, ii))
                if e is not None and e.type in (TYPE_NEVER, TYPE_IMMEDIATE):
                    rect[...] = palette.entries[0 if e.type == TYPE_NEVER else 1]
                    continue
                if e is not None:
                    stream = source.load_serialized(e)
            else:
                stream = fetch_chunk_stream(addr, port, level, ir, ii)
            if stream is None:
                rect[...] = np.asarray(missing, np.uint8)
                missing_chunks.append((ir, ii))
                continue
            dev.render_chunk(stream, palette=palette, scale=scale, out=rect, pitch=width)
    return out, missing_chunks


def main(argv=None, dev=None) -> int:
    """The command line; `dev` (for callers that hold a device already) replaces the MandelbrotDevice it would open."""
    ap = argparse.ArgumentParser(prog="python -m distributedmandelbrot_amd.viewer", description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--store", metavar="DIR", help="parent directory of a chunk store (holds Data/_index.dat)")
    src.add_argument("--server", metavar="ADDR:PORT", help="a DataServer")
    ap.add_argument("--level", type=int, required=True)
    ap.add_argument("--region", metavar="IR0,II0,NR,NI", help="whole chunks; default: the whole level")
    ap.add_argument("--scale", type=int, default=16, choices=L.CHUNK_SCALES)
    ap.add_argument("--palette", choices=("viewer", "cosine"), default="viewer")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("out", metavar="OUT.png")
    args = ap.parse_args(argv)
    if args.store:
        source: Source = ChunkStore(args.store)
    else:
        addr, _, port = args.server.rpartition(":")
        source = (addr, int(port))
    region = tuple(int(v) for v in args.region.split(",")) if args.region else None
    if region is not None and len(region) != 4:
        ap.error("--region takes IR0,II0,NR,NI")
    palette = Palette.viewer() if args.palette == "viewer" else Palette(Palette.cosine(256).entries)
    if dev is not None:
        rgba, missing = render_level(dev, source, args.level, region=region, scale=args.scale, palette=palette)
        write_png(args.out, rgba)
    else:
        from .device import MandelbrotDevice
        with MandelbrotDevice(args.device) as own:   # (the image is pinned memory of the device: written before it closes)
            rgba, missing = render_level(own, source, args.level, region=region, scale=args.scale, palette=palette)
            write_png(args.out, rgba)
    print(f"{args.out}: {rgba.shape[1]} x {rgba.shape[0]} pixels, {len(missing)} chunks missing", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
