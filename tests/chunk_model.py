"""The stored-chunk contract of include/mbk.h ("Stored chunks") in numpy: stream in, bytes / RGBA8 out.  Written from the
header's text, not from the C code: the stream rules as a chain of tests in the header's order, decode = validate + np.repeat,
colour + resolve in per-channel integers.  Below the model: the streams the CPU and the GPU tests share (one invalid stream per
reason code and boundary, and valid but unusual ones)."""

import numpy as np

CHUNK = 4096 * 4096
DIM = 4096
SCALES = (1, 2, 4, 8, 16, 32, 64)
OK, BAD_CODEC, BAD_SIZE, ZERO_RUN, TOO_LONG, TOO_SHORT = range(6)
REASON_NAMES = ["MBK_STREAM_OK", "MBK_STREAM_BAD_CODEC", "MBK_STREAM_BAD_SIZE", "MBK_STREAM_ZERO_RUN", "MBK_STREAM_TOO_LONG",
                "MBK_STREAM_TOO_SHORT"]
RECORD = np.dtype([("len", "<u4"), ("val", "u1")])


class StreamInvalid(ValueError):
    def __init__(self, reason):
        super().__init__(REASON_NAMES[reason])
        self.reason = reason


def check(stream, n=CHUNK):
    """(codec, runs, records) of a valid stream; StreamInvalid(reason) otherwise -- the first reason of the header's list."""
    stream = bytes(stream)
    size = len(stream)
    if size == 0 or not 1 <= n <= CHUNK:
        raise StreamInvalid(BAD_SIZE)
    if stream[0] not in (0, 1):
        raise StreamInvalid(BAD_CODEC)
    if stream[0] == 0:
        if size < 1 + n:
            raise StreamInvalid(BAD_SIZE)
        return 0, 0, None
    if (size - 1) % 5 != 0 or size > 1 + n:
        raise StreamInvalid(BAD_SIZE)
    rec = np.frombuffer(stream, RECORD, offset=1)
    if (rec["len"] == 0).any():
        raise StreamInvalid(ZERO_RUN)
    total = sum(int(v) for v in rec["len"])        # Python integers: no width at all
    if total > n:
        raise StreamInvalid(TOO_LONG)
    if total < n:
        raise StreamInvalid(TOO_SHORT)
    return 1, len(rec), rec


def decode(stream, n=CHUNK):
    codec, _, rec = check(stream, n)
    if codec == 0:
        return np.frombuffer(bytes(stream), np.uint8, count=n, offset=1).copy()
    return np.repeat(rec["val"], rec["len"].astype(np.int64))


def maximal_runs(byts):
    b = np.asarray(byts, np.uint8).ravel()
    return 1 + int(np.count_nonzero(b[1:] != b[:-1]))


def resolve(palette, k, byts):
    """(4096 / k, 4096 / k, 4) uint8: per channel (2 S + k^2) // (2 k^2), S the sum of palette[b] over the pixel's k x k bytes."""
    palette = np.asarray(palette, np.uint8)
    assert palette.shape == (256, 4) and k in SCALES
    b = np.asarray(byts, np.uint8).reshape(DIM, DIM)
    w = DIM // k
    out = np.empty((w, w, 4), np.uint8)
    for c in range(4):
        total = palette[:, c][b].reshape(w, k, w, k).sum(axis=(1, 3), dtype=np.int64)   # one channel at a time: 16 Mi samples
        v = (2 * total + k * k) // (2 * k * k)
        assert v.min() >= 0 and v.max() <= 255
        out[:, :, c] = v
    return out


def mosaic(palette, k, chunks, ir0, ii0, nr, ni, missing=(0, 0, 0, 0)):
    """`chunks`: {(ir, ii): bytes | None}.  Chunk (ir, ii) at columns (ir - ir0) w, rows (ii - ii0) w; row 0 the lowest
    imaginary part; None (or absent) -> `missing`."""
    w = DIM // k
    img = np.empty((ni * w, nr * w, 4), np.uint8)
    for ii in range(ii0, ii0 + ni):
        for ir in range(ir0, ir0 + nr):
            b = chunks.get((ir, ii))
            img[(ii - ii0) * w:(ii - ii0 + 1) * w, (ir - ir0) * w:(ir - ir0 + 1) * w] = \
                np.asarray(missing, np.uint8) if b is None else resolve(palette, k, b)
    return img


# ---- the streams the tests share -----------------------------------------------------------------------------------------

def rle_stream(lengths, values):
    rec = np.zeros(len(lengths), RECORD)
    rec["len"] = np.asarray(lengths, np.uint64).astype(np.uint32)
    rec["val"] = values
    return bytes([1]) + rec.tobytes()


def _split(n, runs, seed):
    """`runs` positive lengths that sum to n, and values (neighbours may be equal: runs need not be maximal)."""
    rs = np.random.RandomState(seed)
    cand = np.unique(rs.randint(1, n, 4 * runs))
    assert len(cand) >= runs - 1
    cuts = np.sort(rs.permutation(cand)[:runs - 1])
    lens = np.diff(np.concatenate(([0], cuts, [n])))
    return [int(v) for v in lens], [int(v) for v in rs.randint(0, 256, runs)]


def invalid_streams(n, runs=3):
    """[(name, stream, reason)] for a chunk of n >= 64 bytes.  The RLE cases hold `runs` (>= 3) records unless the case
    says otherwise; with thousands of them the zero run / the wrong total sit in a later block of the device's scan."""
    assert n >= 64 and 3 <= runs <= n // 8
    lens, vals = _split(n, runs, 5)
    mid = runs // 2

    def mutated(at, delta):
        m = list(lens)
        m[at] += delta
        return rle_stream(m, vals)

    def with_zero(at):      # a zero run inserted, the total still n
        m, v = list(lens), list(vals)
        m.insert(at, 0)
        v.insert(at, 7)
        return rle_stream(m, v)

    good = rle_stream(lens, vals)
    big = 0xffffffff
    out = [
        ("zero_run_first", with_zero(0), ZERO_RUN),
        ("zero_run_last", with_zero(runs), ZERO_RUN),
        ("zero_run_middle", with_zero(mid), ZERO_RUN),
        ("zero_run_and_too_long", rle_stream([0] + lens[:-1] + [lens[-1] + 9], [1] + vals), ZERO_RUN),
        ("sum_n_plus_1", mutated(mid, +1), TOO_LONG),
        ("sum_n_minus_1", mutated(runs - 1, -1) if lens[-1] > 1 else mutated(int(np.argmax(lens)), -1), TOO_SHORT),
        ("sum_wraps_2_32", rle_stream([big, 2] + lens[2:], vals), TOO_LONG),                  # 2^32 + 1 + ...: small mod 2^32
        ("sum_wraps_onto_n", rle_stream([big, n + 1 - sum(lens[2:])] + lens[2:], vals), TOO_LONG),   # == n mod 2^32
        ("raw_one_byte_short", bytes([0]) + bytes(n - 1), BAD_SIZE),
        ("codec_2", bytes([2]) + good[1:], BAD_CODEC),
        ("codec_255_raw_sized", bytes([255]) + bytes(n), BAD_CODEC),
        ("size_0", b"", BAD_SIZE),
        ("size_1_rle", bytes([1]), TOO_SHORT),
        ("size_1_raw", bytes([0]), BAD_SIZE),
        ("one_record_too_short", rle_stream([n - 1], [3]), TOO_SHORT),
        ("one_record_too_long", rle_stream([n + 1], [3]), TOO_LONG),
        ("one_record_zero", rle_stream([0], [3]), ZERO_RUN),
    ]
    for extra in (1, 2, 3, 4):
        out.append((f"payload_5r_plus_{extra}", good + bytes(extra), BAD_SIZE))
    return out


def oversized_rle_stream():
    """The one documented exception: an RLE stream longer than 1 + n whose runs sum to n (n = 10: three records, 16 bytes).
    chunkstore.deserialize_chunk decodes it; the library refuses it with BAD_SIZE.  Returns (stream, n, decoded)."""
    return rle_stream([3, 3, 4], [9, 8, 7]), 10, np.repeat(np.array([9, 8, 7], np.uint8), [3, 3, 4])


def unusual_valid_streams(n, runs=3):
    """[(name, stream, decoded)]: non-maximal runs, Raw with trailing bytes -- and, for n = 10, an RLE stream of exactly 1 + n."""
    lens, vals = _split(n, runs, 11)
    vals[1] = vals[0]                          # two neighbours of equal value
    rs = np.random.RandomState(12)
    raw = rs.randint(0, 256, n, dtype=np.uint8)
    out = [("non_maximal_runs", rle_stream(lens, vals), np.repeat(np.array(vals, np.uint8), lens)),
           ("all_one_value_in_many_runs", rle_stream(lens, [5] * runs), np.full(n, 5, np.uint8)),
           ("raw_with_trailing_bytes", bytes([0]) + raw.tobytes() + b"trailing", raw)]
    if n == 10:
        out.append(("rle_of_exactly_1_plus_n", rle_stream([5, 5], [1, 2]), np.repeat(np.array([1, 2], np.uint8), 5)))
    return out


def tie_chunk_and_palette(seed=21):
    """A chunk and a palette whose every k x k block (k >= 2) has a mean of exactly x.5 in every channel: columns alternate
    between bytes 2 v and 2 v + 1 (v constant over 64 x 64 bytes), and palette[2 v + 1] = palette[2 v] + 1."""
    rs = np.random.RandomState(seed)
    v = np.repeat(np.repeat(rs.randint(0, 128, (64, 64)), 64, axis=0), 64, axis=1)
    byts = (2 * v + (np.arange(DIM)[None, :] & 1)).astype(np.uint8)
    pal = np.empty((256, 4), np.uint8)
    pal[0::2] = rs.randint(0, 255, (128, 4))
    pal[1::2] = pal[0::2] + 1
    return byts, pal


def every_value_chunk(seed=22):
    rs = np.random.RandomState(seed)
    b = rs.randint(0, 256, CHUNK, dtype=np.uint8)
    b[:256] = np.arange(256)
    return b


def random_palette(seed=23):
    return np.random.RandomState(seed).randint(0, 256, (256, 4), dtype=np.uint8)
