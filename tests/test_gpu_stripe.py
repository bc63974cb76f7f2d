"""Stripe-average colouring on the GPU (include/mbk.h, "Stripe-average colouring"), held to the numpy model of the contract
(tests/stripe_model.py).

The accumulated state involves no libm call, so the device must store the model's state on every pixel and bit with every kernel
selector; the value takes two logarithms and is held to the correctly rounded value of its expression at that state, one ulp
more than the host twin is allowed.  The counts are compute_view's.  A stripe render is mbk_stripe_resolve_host (held to the numpy
rule by tests/test_stripe.py) of the device's own smooth samples and stripe averages of the s times finer view, banded or not,
whole or windowed.  The launch forms are captured, replayed and run beside each other on two streams.  The shapes are the
smallest at which the kernel can go wrong: ragged against the 8x8 blocks, more than one block, whole-interior blocks, one row.
"""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import stripe_model as SM
from distributedmandelbrot_amd import MandelbrotDevice, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import stripe_state_arrays, stripe_state_host
from distributedmandelbrot_amd.image import stripe_resolve_host
from launch_cases import BLOCKS, RAGGED, RENDER_VIEW, SEAHORSE, Case, Out, _check, _image, _render_palette, _rgba

pytestmark = pytest.mark.gpu

STATE_KEYS = ("S", "t_last", "mag", "N", "cnt")
_MODEL = {}


def _model(v, mrd, density, skip, window=None):
    key = (v, mrd, density, skip, window)
    if key not in _MODEL:
        _MODEL[key] = SM.model(v, mrd, density, skip, window)
    return _MODEL[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_state(got, want):
    return all(_same_bits(got[k], want[k]) for k in ("S", "t_last", "mag")) and all(np.array_equal(got[k], want[k]) for k in ("N", "cnt"))


def _held_to_the_model(counts, v, state, st, mn, what):
    """Counts and state equal the model's on every bit; v within the recorded ulps of the correctly rounded value at that state."""
    assert np.array_equal(counts, mn), what
    for k in ("S", "t_last", "mag"):
        assert _same_bits(state[k], st[k]), (what, k, int((_bits(state[k]) != _bits(st[k])).sum()))
    assert np.array_equal(state["N"], st["N"]) and np.array_equal(state["cnt"], st["cnt"]), what
    assert not np.isnan(v).any() and np.array_equal(v == 0.0, counts == 0), what
    e = SM.value_err_ulps(v, st)
    assert not np.isnan(e).any(), what
    print(f"{what}: {int((mn > 0).sum())} escaped pixels, worst {e.max():.4f} ulp(v) (allowed {SM.VALUE_ULPS_GPU})")
    assert e.max() <= SM.VALUE_ULPS_GPU, (what, float(e.max()))


@pytest.mark.parametrize("kernel,density,skip", [("default", 5, 0), ("scan", 5, 0), ("group", 5, 0), ("default", 1, 3), ("default", 16, 3)])
def test_whole_view_equals_the_model(gpu, kernel, density, skip):
    v, mrd = SEAHORSE
    view = View(*v)
    st, mn, mv = _model(v, mrd, density, skip)
    assert (mn == 0).sum() > 50 and len(np.unique(mn)) > 40
    ref, _, _ = gpu.compute_view(view, mrd, want_bytes=False)
    counts, val, state, stats = gpu.compute_view_stripes(view, mrd, density=density, skip=skip, kernel=kernel, want_state=True)
    assert counts.dtype == np.int32 and val.dtype == np.float64 and val.shape == (45, 67) and np.array_equal(counts, ref)
    _held_to_the_model(counts, val, state, st, mn, f"{kernel}, density {density}, skip {skip}")
    assert stats.pixel_iterations == int(np.where(counts > 0, counts, mrd - 1).astype(np.int64).sum())
    assert stats.never_pixels == int((counts == 0).sum())
    # without the state: the same values
    c2, v2, _ = gpu.compute_view_stripes(view, mrd, density=density, skip=skip, kernel=kernel)
    assert np.array_equal(c2, counts) and _same_bits(v2, val)
    assert (val[counts > 0] > 0.0).all() and (val[counts > 0] < 1.0).all() and val[counts > 0].std() > 0.01


def test_view_with_whole_interior_blocks(gpu):
    v, mrd = BLOCKS
    st, mn, _ = _model(v, mrd, 5, 0)
    blocks = (mn.reshape(8, 8, 8, 8) == 0).all(axis=(1, 3))
    assert blocks.sum() >= 8 and (mn > 0).sum() > 500 and not blocks.all()
    counts, val, state, _ = gpu.compute_view_stripes(View(*v), mrd, want_state=True)
    _held_to_the_model(counts, val, state, st, mn, "64 x 64 with whole-interior blocks")


def test_window_equals_the_same_pixels_of_the_whole_view(gpu):
    v, mrd = (-2.0, -1.25, 2.75, 2.5, 128, 96), 300
    view = View(*v)
    wc, whole, wstate, _ = gpu.compute_view_stripes(view, mrd, want_state=True)
    assert (wc == 0).any() and len(np.unique(wc)) > 20
    c0, r0, nc, nr = window = (5, 3, 21, 17)
    c, val, state, stats = gpu.compute_view_stripes(view, mrd, window=window, want_state=True)
    cut = (slice(r0, r0 + nr), slice(c0, c0 + nc))
    assert np.array_equal(c, wc[cut]) and _same_bits(val, whole[cut])
    assert _same_state(state, {k: wstate[k][cut] for k in STATE_KEYS})
    assert stats.pixel_iterations == int(np.where(c > 0, c, mrd - 1).astype(np.int64).sum())
    st, mn, _ = _model(v, mrd, 5, 0, window)
    _held_to_the_model(c, val, state, st, mn, "window")


def test_other_shapes(gpu):
    row = (-2.0, 0.3, 2.5, 0.0, 33, 1)                      # a single row
    c, val, state, _ = gpu.compute_view_stripes(View(*row), 200, density=5, skip=1, want_state=True)
    st, mn, _ = _model(row, 200, 5, 1)
    assert (mn > 0).sum() > 5
    _held_to_the_model(c, val, state, st, mn, "33 x 1")
    v = (-2.0, -2.0, 4.0, 4.0, 16, 16)
    for mrd in (0, 1, 2):
        c, val, state, stats = gpu.compute_view_stripes(View(*v), mrd, want_state=True)
        st, mn, _ = _model(v, mrd, 5, 0)
        _held_to_the_model(c, val, state, st, mn, f"mrd {mrd}")
        if mrd < 2:
            assert not c.any() and not val.any() and not any(state[k].any() for k in STATE_KEYS)
            assert stats.pixel_iterations == 0 and stats.never_pixels == 256
        else:
            assert set(np.unique(c)) == {0, 1} and (val[c == 1] > 0.0).all()
    # skip past every orbit: 0.5 wherever something escaped
    c, val, state, _ = gpu.compute_view_stripes(View(*SEAHORSE[0]), SEAHORSE[1], skip=2 ** 31 - 1, want_state=True)
    assert (val[c > 0] == 0.5).all() and not val[c == 0].any() and not state["cnt"].any() and not state["S"].any()


def test_special_pixels_store_what_the_host_twin_stores(gpu):
    # the first pixel is exactly -2 + 0i: n = 1, the run-on takes all its 64 steps, d clamps to 1
    line = (-2.0, 0.0, 1.0, 0.5, 9, 3)
    # mag = inf at the first step, the term 0.5.  The host twin is held to this at c = 1e200 (tests/test_stripe.py); a view cannot
    # hold 1e200 -- every view call refuses coordinates above 2^500, the stripe calls with them (asserted below) -- so the view
    # holds 2^500, the largest coordinate a view takes: z_1 = 2^1000 is finite and fl(zr^2) = +inf, the same branch.
    big = (0.0, 0.0, 2.0 ** 500, 0.5, 9, 3)
    with pytest.raises(MbkError):
        gpu.compute_view_stripes(View(-1e200, -1e200, 2e200, 2e200, 9, 3), 100)
    for v, at, N in ((line, (0, 0), 65), (big, (0, 8), 1)):
        for density in (1, 5, 16):
            c, val, state, _ = gpu.compute_view_stripes(View(*v), 100, density=density, want_state=True)
            st, mn, _ = _model(v, 100, density, 0)
            _held_to_the_model(c, val, state, st, mn, f"{v[0]}, density {density}")
            cr, ci = SM.DM.axes(v)
            for r in range(3):
                for col in range(9):
                    h = stripe_state_host((cr[col], ci[r]), 100, density=density)
                    got = {k: state[k][r, col].item() for k in STATE_KEYS}
                    assert h["n"] == c[r, col] and all(got[k] == h[k] for k in STATE_KEYS), (v, r, col, h, got)
                    assert abs(val[r, col] - h["v"]) <= 4.0 * np.spacing(abs(h["v"]))
            assert c[at] == 1 and state["N"][at] == N and val[at] == 0.5 and not np.isnan(val).any()
            if v is big:
                assert state["mag"][at] == math.inf and (state["mag"][:, 1:] == math.inf).all() and (c[:, 1:] == 1).all()
    assert SM.DM.axes(line)[0][0] == -2.0 and SM.DM.axes(line)[1][0] == 0.0 and SM.DM.axes(big)[0][8] == 2.0 ** 500


def _stripes(v, mrd, *, density=5, skip=0, kernel="default", window=None, with_counts=True, with_state=True) -> Case:
    """mbk_view_launch_stripe as a catalogue case (tests/launch_cases.py): the state buffer as 4 px binary64 words."""
    view = View(*v)
    n = window[2] * window[3] if window is not None else v[4] * v[5]

    def want(dev):
        c, val, state, _ = dev.compute_view_stripes(view, mrd, density=density, skip=skip, kernel=kernel, window=window, want_state=True)
        raw = np.concatenate([state[k].ravel().view(np.uint8) for k in STATE_KEYS]).view(np.float64)
        out = {"stripe": val}
        if with_counts:
            out["counts"] = c
        if with_state:
            out["state"] = raw
        return out
    return Case(lambda: {"stripe": Out("f8", n), "counts": Out("i4", n), "state": Out("f8", 4 * n)},
                lambda dev, o, s: dev.launch_view_stripes(view, mrd, d_stripe=o["stripe"].ptr, d_counts=o["counts"].ptr if with_counts else 0,
                                                          d_state=o["state"].ptr if with_state else 0, density=density, skip=skip, stream=s,
                                                          window=window, kernel=kernel), want)


def _stripe_render(pal, *, s=2, rows=0, window=None, density=5, skip=0, lo=0.25, gain=1.5, kernel="default") -> Case:
    v, mrd = RENDER_VIEW
    view = View(*v)
    n = window[2] * window[3] if window is not None else v[4] * v[5]
    kw = dict(palette=pal, density=density, skip=skip, lo=lo, gain=gain, supersample=s, window=window, max_band_rows=rows, kernel=kernel)
    return Case(_image(n), lambda dev, o, st: dev.launch_render_view_stripes(view, mrd, d_rgba=o["rgba"].ptr, stream=st, **kw),
                lambda dev: _rgba(dev.render_view_stripes(view, mrd, **kw)[0]))


@pytest.mark.parametrize("kernel", ["default", "scan", "group"])
def test_launch_writes_every_element_and_nothing_else(gpu, kernel):
    """The launch form on a torch stream into sentinel-filled buffers with guard elements on both sides, on the whole 64 x 64
    view with whole-interior blocks and on a ragged window; d_counts = NULL and d_state = NULL each work."""
    import torch
    v, mrd = BLOCKS
    stream = torch.cuda.Stream(device="cuda:0")
    for window in (None, RAGGED):
        st, mn, _ = _model(v, mrd, 5, 0, window)
        for with_counts, with_state in ((True, True), (False, True), (True, False), (False, False)):
            case = _stripes(v, mrd, kernel=kernel, window=window, with_counts=with_counts, with_state=with_state)
            outs = case.outs()
            torch.cuda.synchronize()
            case.launch(gpu, outs, stream.cuda_stream)
            stream.synchronize()
            _check(outs, case.want(gpu), (kernel, window, with_counts, with_state))
            if with_state:
                state = stripe_state_arrays(outs["state"].body().view(np.uint8), mn.shape)
                val = outs["stripe"].body().reshape(mn.shape)
                _held_to_the_model(mn, val, state, st, mn, f"launch, {kernel}, window {window}")
                assert not val[mn == 0].any() and not np.signbit(val[mn == 0]).any()       # zeros, written


def _finer(view, s):
    return View(view.start_r, view.start_i, view.range_r, view.range_i, view.width * s, view.height * s)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_render_equals_the_host_rule_and_the_model(gpu, s):
    v, mrd = SEAHORSE[0], 400
    view = View(*v)
    w, h = view.width, view.height
    pal = _render_palette()
    fine = _finer(view, s)
    density, skip, lo, gain = 5, 2, 0.25, 1.5
    nu, counts, st_s = gpu.compute_view_smooth(fine, mrd)
    c2, val, _ = gpu.compute_view_stripes(fine, mrd, density=density, skip=skip)
    assert np.array_equal(counts, c2) and (counts == 0).any() and len(np.unique(counts)) > 10
    want = stripe_resolve_host(pal, s, w, h, counts=counts, smooth=nu, stripe=val, density=density, skip=skip, lo=lo, gain=gain)
    model = SM.render(pal.entries, pal.inside, pal.scale, pal.offset, lo, gain, s, counts, nu, val)
    assert np.array_equal(want, model) and len(np.unique(want.reshape(-1, 4), axis=0)) > 100
    kw = dict(palette=pal, density=density, skip=skip, lo=lo, gain=gain, supersample=s)
    for rows in (0, 7):
        img, st = gpu.render_view_stripes(view, mrd, max_band_rows=rows, **kw)
        assert img.shape == (h, w, 4) and np.array_equal(img, want), (rows, int((img != want).any(axis=2).sum()))
        assert (st.pixel_iterations, st.never_pixels) == (st_s.pixel_iterations, st_s.never_pixels)
    window = (7, 5, 19, 13)
    img, _ = gpu.render_view_stripes(view, mrd, window=window, **kw)
    assert np.array_equal(img, want[5:18, 7:26])
    img, _ = gpu.render_view_stripes(view, mrd, window=window, max_band_rows=7, **kw)
    assert np.array_equal(img, want[5:18, 7:26])
    # the stripes are there: the image differs from the neutral one, and lo = 1 is the smooth render
    flat, _ = gpu.render_view_stripes(view, mrd, palette=pal, density=density, skip=skip, lo=lo, gain=0.0, supersample=s)
    assert (flat != want).any(axis=2).sum() > 200
    smooth, _ = gpu.render_view(view, mrd, palette=pal, source="smooth", supersample=s)
    assert np.array_equal(gpu.render_view_stripes(view, mrd, palette=pal, density=density, lo=1.0, gain=gain, supersample=s)[0], smooth)
    # the launch form on a caller's stream, guard words behind the image
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    d = torch.zeros(h * w + 256, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_view_stripes(view, mrd, d_rgba=d.data_ptr(), stream=stream.cuda_stream, max_band_rows=7, **kw)
    stream.synchronize()
    hd = d.cpu().numpy()
    assert np.array_equal(hd[:h * w].view(np.uint8).reshape(h, w, 4), want) and not hd[h * w:].any()


# ---- graph capture (include/mbk.h, "Graph capture"): the pattern of tests/test_gpu_graph.py --------------------------------------

def _capture(torch, s, enqueue):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue()
    torch.cuda.synchronize()
    return g


def _replay(torch, s, g):
    with torch.cuda.stream(s):
        g.replay()
    s.synchronize()


def _drop(g):
    g.reset()
    del g
    gc.collect()


def _refill(torch, outs):
    for o in outs.values():
        o.refill()
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["values", "render"])
def test_capture_and_three_replays(form):
    """One warm call, one capture, three replays, each held to the synchronous form's bytes; between the first and the second
    another launch of the family runs on the stream, through the same count and render scratch."""
    import torch
    pal = _render_palette()
    if form == "values":
        case, inter = _stripes(*SEAHORSE, with_counts=False), _stripes(*SEAHORSE, density=3, skip=2, window=RAGGED, with_counts=False)
    else:
        case, inter = _stripe_render(pal, s=2, rows=10), _stripe_render(pal, s=1, window=(7, 5, 19, 13), density=2)
    with MandelbrotDevice(0) as dev:
        s = torch.cuda.Stream(device="cuda:0")
        want, iwant = case.want(dev), inter.want(dev)
        A, B, I = case.outs(), case.outs(), inter.outs()
        torch.cuda.synchronize()
        case.launch(dev, A, s.cuda_stream)
        s.synchronize()
        _check(A, want, "warm call")
        g = _capture(torch, s, lambda: case.launch(dev, B, s.cuda_stream))
        try:
            assert all(o.untouched() for o in B.values()), "a capture runs nothing"
            _replay(torch, s, g)
            _check(B, want, "replay 1")
            _refill(torch, B)
            inter.launch(dev, I, s.cuda_stream)
            _replay(torch, s, g)
            _check(B, want, "replay 2, behind another launch on the stream")
            _check(I, iwant, "the interposed launch")
            _refill(torch, B)
            _replay(torch, s, g)
            _check(B, want, "replay 3")
        finally:
            _drop(g)
        assert len(np.unique(_bytes_of(want))) > 50


def _bytes_of(want):
    return np.concatenate([np.ascontiguousarray(a).ravel().view(np.uint8) for a in want.values()])


@pytest.mark.parametrize("form", ["values", "render"])
def test_cold_capture_raises_and_leaves_the_capture_usable(form):
    """The first call of a ctx on a stream allocates its scratch: inside a capture it raises before it enqueues anything, the
    stream is still capturing, a launch that needs nothing of the ctx is captured behind it and replays, and the refused call
    succeeds outside the capture."""
    import torch
    from launch_cases import plain
    pal = _render_palette()
    bad = _stripes(*SEAHORSE, with_counts=False) if form == "values" else _stripe_render(pal)
    good = plain(SEAHORSE[0], SEAHORSE[1], "default", "counts")
    with MandelbrotDevice(0) as dev:
        s = torch.cuda.Stream(device="cuda:0")
        gwant = good.want(dev)
        R, B = bad.outs(), good.outs()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(MbkError) as err:
                bad.launch(dev, R, s.cuda_stream)
            still = torch.cuda.is_current_stream_capturing()
            good.launch(dev, B, s.cuda_stream)
        torch.cuda.synchronize()
        try:
            assert still, "the refusal ended the capture"
            assert err.value.status == 1 and "graph capture:" in str(err.value) and "first call" in str(err.value), str(err.value)
            assert all(o.untouched() for o in R.values()) and all(o.untouched() for o in B.values())
            _replay(torch, s, g)
            _check(B, gwant, "the launch captured behind the refusal")
            assert all(o.untouched() for o in R.values())
        finally:
            _drop(g)
        bad.launch(dev, R, s.cuda_stream)
        s.synchronize()
        _check(R, bad.want(dev), "the refused call, outside the capture")


# ---- streams (include/mbk.h, "Streams"): the pattern of tests/test_gpu_streams.py ---------------------------------------------

BALLAST_MS = 10.0      # as tests/test_gpu_streams.py: many times the host time of the four enqueues below


def _cycles_per_ms(torch) -> float:
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    n = 1_000_000
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0 or n >= 10 ** 11:
            return n / ms
        n *= 10


def test_both_launch_forms_beside_each_other_on_two_streams():
    """The value launch (counts in the stream's scratch) and the render launch, each on both streams, queued behind a ballast so
    that they start together; every output holds the bytes the synchronous form stores on a device of its own."""
    import torch
    pal = _render_palette()
    cases = [_stripes(*SEAHORSE, with_counts=False), _stripe_render(pal, s=2, rows=10),
             _stripe_render(pal, s=2, rows=10), _stripes(*SEAHORSE, with_counts=False)]
    with MandelbrotDevice(0) as ref:
        wants = [c.want(ref) for c in cases]
    with MandelbrotDevice(0) as dev:
        streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
        assert streams[0].cuda_stream != streams[1].cuda_stream
        outs = [c.outs() for c in cases]
        for k, c in enumerate(cases):      # warm: each stream brings its scratch and its palette
            c.launch(dev, outs[k], streams[k % 2].cuda_stream)
        torch.cuda.synchronize()
        for k, w in enumerate(wants):
            _check(outs[k], w, f"alone, case {k}")
            _refill(torch, outs[k])
        cycles = int(_cycles_per_ms(torch) * BALLAST_MS)
        events = []
        for s in streams:
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
            e = torch.cuda.Event()
            e.record(s)
            events.append(e)
        for k, c in enumerate(cases):      # stream 0: values, render; stream 1: render, values
            c.launch(dev, outs[k], streams[k % 2].cuda_stream)
        pending = [not e.query() for e in events]
        for s in streams:
            s.synchronize()
        assert all(pending), "a ballast ended before the last enqueue: nothing proves that the launches overlap"
        for k, w in enumerate(wants):
            _check(outs[k], w, f"beside the others, case {k}")


def test_refusals_leave_the_output_untouched(gpu):
    import torch
    view = View(-2.0, -2.0, 4.0, 4.0, 16, 16)
    cv = gpu._cview(view, None)
    outs = {"stripe": Out("f8", 256), "counts": Out("i4", 256), "state": Out("f8", 1024), "rgba": Out("rgba", 256)}
    torch.cuda.synchronize()
    pv, pc, ps, pi = (outs[k].ptr for k in ("stripe", "counts", "state", "rgba"))
    launch = gpu._lib.mbk_view_launch_stripe
    assert launch(gpu._h, C.byref(cv), 100, L.MBK_KERNEL_DEFAULT, 5, 0, pc, None, ps, None) == L.MBK_ERR_INVALID       # NULL values
    with pytest.raises(MbkError):
        gpu.launch_view_stripes(view, 100, d_stripe=0, d_counts=pc)
    for kernel in ("default", "scan", "group"):
        for flag in (L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, 0x1, 0x2, 0x4000, 0x80000000):
            assert launch(gpu._h, C.byref(cv), 100, L.KERNELS[kernel] | flag, 5, 0, pc, pv, ps, None) == L.MBK_ERR_INVALID, (kernel, flag)
    for kernel in ("simple", "refill", "asm"):      # "asm": there is no one-pass form
        with pytest.raises(MbkError):
            gpu.launch_view_stripes(view, 100, d_stripe=pv, d_counts=pc, kernel=kernel)
        with pytest.raises(MbkError):
            gpu.compute_view_stripes(view, 100, kernel=kernel)
    assert launch(gpu._h, C.byref(cv), 100, 0x600, 5, 0, pc, pv, ps, None) == L.MBK_ERR_INVALID                         # unknown selector
    for density in (0, 17, 2 ** 31, 2 ** 32 - 1):
        assert launch(gpu._h, C.byref(cv), 100, 0, density, 0, pc, pv, ps, None) == L.MBK_ERR_INVALID, density
    assert launch(gpu._h, C.byref(cv), 100, 0, 5, 2 ** 31, pc, pv, ps, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.compute_view_stripes(view, 100, density=0)
    with pytest.raises(MbkError):
        gpu.launch_view_stripes(view, 2 ** 31, d_stripe=pv)
    with pytest.raises(MbkError):
        gpu.launch_view_stripes(view, 100, d_stripe=pv, window=(10, 0, 7, 16))
    with pytest.raises(MbkError):
        gpu.launch_view_stripes(View(2.0 ** 500, 0.0, 2.0 ** 500, 1.0, 4, 4), 100, d_stripe=pv)
    assert launch(gpu._h, None, 100, L.MBK_KERNEL_DEFAULT, 5, 0, None, pv, None, None) == L.MBK_ERR_INVALID
    hv, hc = np.full(256, -1.0), np.full(256, -3, np.int32)
    compute = gpu._lib.mbk_view_compute_stripe
    assert compute(gpu._h, C.byref(cv), 100, 0, 5, 0, hc.ctypes.data, None, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, None, 100, 0, 5, 0, hc.ctypes.data, hv.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 100, L.MBK_PRECISION_F32, 5, 0, hc.ctypes.data, hv.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 100, L.KERNELS["asm"], 5, 0, hc.ctypes.data, hv.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 100, 0, 17, 0, hc.ctypes.data, hv.ctypes.data, None, None) == L.MBK_ERR_INVALID
    assert compute(gpu._h, C.byref(cv), 2 ** 31, 0, 5, 0, hc.ctypes.data, hv.ctypes.data, None, None) == L.MBK_ERR_INVALID
    # the render calls: what a smooth render refuses, and the spec's own ranges
    pal = _render_palette()
    rl, rc = gpu._lib.mbk_view_stripe_render_launch, gpu._lib.mbk_view_stripe_render_compute
    himg = np.full((16, 16, 4), 7, np.uint8)
    ok = pal.stripe_spec(1)
    bad_specs = [pal.stripe_spec(5), pal.stripe_spec(1, density=0), pal.stripe_spec(1, density=17), pal.stripe_spec(1, skip=2 ** 31),
                 pal.stripe_spec(1, lo=-0.5), pal.stripe_spec(1, lo=1.5), pal.stripe_spec(1, lo=math.nan), pal.stripe_spec(1, lo=math.inf),
                 pal.stripe_spec(1, gain=-0.5), pal.stripe_spec(1, gain=2.0 ** 10 + 1), pal.stripe_spec(1, gain=math.nan),
                 pal.stripe_spec(1, gain=math.inf), Palette(pal.entries[:1]).stripe_spec(1), Palette(pal.entries, scale=0.0).stripe_spec(1),
                 Palette(pal.entries, scale=2.0 ** 21).stripe_spec(1), Palette(pal.entries, offset=math.nan).stripe_spec(1)]
    no_palette = pal.stripe_spec(1)
    no_palette.palette = None
    for spec in bad_specs + [no_palette]:
        assert rl(gpu._h, C.byref(cv), 100, 0, C.byref(spec), pi, None) == L.MBK_ERR_INVALID
        assert rc(gpu._h, C.byref(cv), 100, 0, C.byref(spec), himg.ctypes.data, None) == L.MBK_ERR_INVALID
    assert rl(gpu._h, C.byref(cv), 100, 0, None, pi, None) == rc(gpu._h, C.byref(cv), 100, 0, None, himg.ctypes.data, None) == L.MBK_ERR_INVALID
    assert rl(gpu._h, C.byref(cv), 100, 0, C.byref(ok), None, None) == rc(gpu._h, C.byref(cv), 100, 0, C.byref(ok), None, None) == L.MBK_ERR_INVALID
    assert rl(gpu._h, None, 100, 0, C.byref(ok), pi, None) == L.MBK_ERR_INVALID
    for flags in (L.MBK_PRECISION_F32, L.KERNELS["simple"], L.KERNELS["refill"], 0x600, L.MBK_LAZY_UNIFORM, 0x1):
        assert rl(gpu._h, C.byref(cv), 100, flags, C.byref(ok), pi, None) == L.MBK_ERR_INVALID, flags
        assert rc(gpu._h, C.byref(cv), 100, flags, C.byref(ok), himg.ctypes.data, None) == L.MBK_ERR_INVALID, flags
    assert rl(gpu._h, C.byref(cv), 2 ** 31, 0, C.byref(ok), pi, None) == L.MBK_ERR_INVALID
    with pytest.raises(MbkError):
        gpu.render_view_stripes(view, 100, palette=pal, window=(10, 0, 7, 16))
    with pytest.raises(MbkError):
        gpu.render_view_stripes(view, 100, palette=pal, gain=-1.0)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values())
    assert (himg == 7).all() and (hv == -1.0).all() and (hc == -3).all()
    # and the accepted calls right after them work
    out, _ = gpu.render_view_stripes(view, 100, palette=pal)
    assert out.shape == (16, 16, 4)
    c, val, _ = gpu.compute_view_stripes(view, 100)
    assert (c > 0).any() and (val[c > 0] > 0.0).all()
