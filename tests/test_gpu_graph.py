"""Graph capture and replay of the launch forms (include/mbk.h, "Graph capture"; DESIGN.md, "Graph capture").

Every other GPU test of a *_launch form issues it, synchronises and compares.  That shape cannot see host-side state that a launch
consumes at enqueue time and a replay does not refresh (which dispatch list, which cursor set, which time-stamp slot), work that
leaves the caller's stream, or a hidden synchronisation, allocation or synchronous copy on a path the header calls asynchronous.
A capture in torch's default (global) error mode is invalidated by any such call, and a replay around other launches of the same
ctx on the same stream stores something else if a launch depended on state of its enqueue.

The pattern of a capturable case (_cycle): the launch once outside a capture into A, which must hold the bits of the synchronous
form; the same launch captured into a sentinel-filled B with guard elements around it -- nothing may be written, a capture runs
nothing; a replay: B holds A's bits and the guards are intact; another launch of the family on the same stream (one that takes a
dispatch list, a cursor set, or the count / render scratch), then a replay: B again, and the interposed launch's own output is
right; a third replay.  Accumulating calls (histograms, density) add once per replay instead.  A refusal (_refusal) leaves the
capture valid and writes nothing: the stream is still capturing after it, a launch captured behind it replays correctly, and the
refused call succeeds outside the capture.  Stale graphs are never replayed: the lifetime rules are documented, not provoked.

Every test opens its own MandelbrotDevice, so that no other test grows the scratch under a live graph, and drops its graphs
before the context closes.  The shapes are the smallest at which each path exists; a case is milliseconds of GPU work.
"""
import gc

import numpy as np
import pytest

from distributedmandelbrot_amd import DeepView, MandelbrotDevice, MbkError, Palette
from launch_cases import (BLOCKS, DEEP_KINDS, DENSITY, FULL, INTERIOR, JULIA, RAGGED, RENDERS, SEAHORSE, Case, Out, _check, _deep, _image, _lut,
                          _ordered_mrd, _render_palette, _rgba, _wide, counts_histogram, deep, density, density_render, distance, histogram,
                          interior, julia, julia_distance, normals, plain, render)

pytestmark = pytest.mark.gpu


def _all_untouched(outs) -> bool:
    return all(o.untouched() for o in outs.values())


def _refill(torch, outs) -> None:
    for o in outs.values():
        o.refill()
    torch.cuda.synchronize()


def _capture(torch, s, enqueue):
    """enqueue() captured on the torch stream s in the default (global) error mode, the strictest."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue()
    torch.cuda.synchronize()
    return g


def _replay(torch, s, g) -> None:
    with torch.cuda.stream(s):      # ordered against the ctx' other work on the capture stream (mbk.h)
        g.replay()
    s.synchronize()


def _drop(g) -> None:
    g.reset()
    del g
    gc.collect()


def _cycle(dev, case: Case, inter: Case):
    """Steps 1 to 6 of the module's docstring for an overwriting launch."""
    import torch
    s = torch.cuda.Stream(device="cuda:0")
    want, iwant = case.want(dev), inter.want(dev)
    A, B, I = case.outs(), case.outs(), inter.outs()
    torch.cuda.synchronize()
    case.launch(dev, A, s.cuda_stream)
    s.synchronize()
    _check(A, want, "warm call")
    g = _capture(torch, s, lambda: case.launch(dev, B, s.cuda_stream))
    try:
        assert _all_untouched(B), "a capture runs nothing"
        _replay(torch, s, g)
        _check(B, want, "replay 1")
        _refill(torch, B)
        for _ in range(inter.times):
            inter.launch(dev, I, s.cuda_stream)
        _replay(torch, s, g)
        _check(B, want, "replay 2, behind another launch on the stream")
        _check(I, iwant, "the interposed launch")
        _refill(torch, B)
        _replay(torch, s, g)
        _check(B, want, "replay 3")
    finally:
        _drop(g)


def _cycle_accumulate(dev, case: Case, inter: Case):
    """The same for a call that ADDS into its table: zeroed once, n replays leave n times the single result."""
    import torch
    s = torch.cuda.Stream(device="cuda:0")
    want, iwant = case.want(dev), inter.want(dev)
    A, B, I = case.outs(), case.outs(), inter.outs()
    for outs in (A, B, I):
        for o in outs.values():
            o.zero_body()
    torch.cuda.synchronize()
    case.launch(dev, A, s.cuda_stream)
    s.synchronize()
    _check(A, want, "warm call")
    assert all(np.asarray(w).any() for w in want.values())
    g = _capture(torch, s, lambda: case.launch(dev, B, s.cuda_stream))
    try:
        _check(B, want, "a capture runs nothing", factor=0)
        _replay(torch, s, g)
        _check(B, want, "replay 1")
        for _ in range(inter.times):
            inter.launch(dev, I, s.cuda_stream)
        _replay(torch, s, g)
        _check(B, want, "replay 2, behind another launch on the stream", factor=2)
        _check(I, iwant, "the interposed launch", factor=inter.times)
        _replay(torch, s, g)
        _check(B, want, "replay 3", factor=3)
    finally:
        _drop(g)


def _refusal(dev, bad: Case, good: Case, text: str):
    """`bad` inside a capture of the stream s: MBK_ERR_INVALID whose message begins "graph capture:" and holds `text`, the stream
    still capturing, nothing written; `good`, captured behind it, replays correctly; then `bad` succeeds outside the capture
    and stores what its synchronous form stores (computed last: that form would bring what the refusal is about).  The warm call
    of `good` is all the ctx has seen on the stream."""
    import torch
    s = torch.cuda.Stream(device="cuda:0")
    gwant = good.want(dev)
    R, B, W = bad.outs(), good.outs(), good.outs()
    torch.cuda.synchronize()
    good.launch(dev, W, s.cuda_stream)
    s.synchronize()
    _check(W, gwant, "warm call")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with pytest.raises(MbkError) as err:
            bad.launch(dev, R, s.cuda_stream)
        still = torch.cuda.is_current_stream_capturing()
        good.launch(dev, B, s.cuda_stream)
    torch.cuda.synchronize()
    try:
        assert still, "the refusal ended the capture"
        assert err.value.status == 1 and "graph capture:" in str(err.value) and text in str(err.value), str(err.value)
        assert _all_untouched(R) and _all_untouched(B)
        _replay(torch, s, g)
        _check(B, gwant, "the launch captured behind the refusal")
        assert _all_untouched(R)
    finally:
        _drop(g)
    bad.launch(dev, R, s.cuda_stream)
    s.synchronize()
    _check(R, bad.want(dev), "the refused call, outside the capture")


@pytest.mark.parametrize("outputs", ["counts+bytes", "bytes", "smooth"])
@pytest.mark.parametrize("kernel", ["default", "group", "asm"])
def test_plain_small_window(kernel, outputs):
    """Under 16 384 blocks every selector is one kernel on the caller's stream.  Interposed: "scan" on a window of the view, whose
    two-pass form takes a cursor set of the stream and turns scan_turn."""
    v, mrd = SEAHORSE
    with MandelbrotDevice(0) as dev:
        _cycle(dev, plain(v, mrd, kernel, outputs), plain(v, mrd, "scan", "counts", window=(3, 5, 40, 33), times=2))


ORDERED = [("default", None), ("group", None), ("asm", None), ("group", "units")]


@pytest.mark.parametrize("cycle_detect", [0, 1])
@pytest.mark.parametrize("prepass_overlap", [0, 1, 2])
@pytest.mark.parametrize("kernel,order", ORDERED, ids=["default", "group", "asm", "units"])
def test_plain_ordered_path(kernel, order, prepass_overlap, cycle_detect):
    """1024 x 1024 = exactly 16 384 blocks of 8 x 8 at the smallest mrd that takes a dispatch list: the pre-pass and the tile kernel
    are two launches tied by a list.  Outside a capture the pre-pass of prepass_overlap 1 / 2 runs on the ctx' auxiliary stream into
    a list of the stream's ring; a captured launch must carry its pre-pass in the graph, into a list no later launch takes.
    Interposed: three launches of the same size on a window of a finer view of the same rectangle, which take every list of the
    ring in turn -- the third replay then runs right behind them.  The expected counts are the same ctx' outside a capture
    (tests/test_gpu_parity.py holds those to the oracle under every option used here)."""
    with MandelbrotDevice(0) as dev:
        dev.set_option("prepass_overlap", prepass_overlap)
        dev.set_option("cycle_detect", cycle_detect)
        if order == "units":
            dev.set_option("order", 3)
            dev.set_option("units_min_light", 0)
        assert dev.get_option("order") >= 2
        mrd = _ordered_mrd(dev)
        case = plain(FULL + (1024, 1024), mrd, kernel, "counts")
        inter = plain(FULL + (2048, 2048), mrd, kernel, "counts", window=(512, 512, 1024, 1024), times=3)
        _cycle(dev, case, inter)
        assert len(np.unique(case.want(dev)["counts"])) > 10


def test_plain_ordered_bytes_and_xcd_balance():
    """The units kernel with MBK_OPT_XCD_BALANCE = 1 (strict loops: where the option applies) and both outputs: inside a capture
    the option acts as 0 -- the time-stamp slot and its tag belong to one enqueue -- and the results are those of every deal."""
    with MandelbrotDevice(0) as dev:
        for name, value in (("order", 3), ("units_min_light", 0), ("xcd_balance", 1), ("cycle_detect", 0)):
            dev.set_option(name, value)
        mrd = _ordered_mrd(dev)
        _cycle(dev, plain(FULL + (1024, 1024), mrd, "group", "counts+bytes"),
               plain(FULL + (2048, 2048), mrd, "group", "counts+bytes", window=(512, 512, 1024, 1024), times=3))


def test_default_selector_where_it_would_take_scan():
    """Outside a capture the default selector takes "scan" where the host probe finds little or nothing heavy.  A window wholly
    outside |c| = 2.5 takes its finish-in-place form -- one kernel, which a capture keeps.  With heavy_share = 65536 ("always
    scan") the full set takes the two-pass form, which a capture replaces by "group": in image order as long as the stream has no
    dispatch lists (the warm call had no reason to grow them), behind the capture list once a "group" launch has."""
    with MandelbrotDevice(0) as dev:
        outside = (-3.5, 1.0, 1.0, 1.0, 1024, 1024)
        _cycle(dev, plain(outside, 300, "default", "counts"), plain(outside, 300, "scan", "counts", window=(0, 0, 512, 512)))
        assert (plain(outside, 300, "default", "counts").want(dev)["counts"] == 1).all()
    with MandelbrotDevice(0) as dev:
        dev.set_option("heavy_share", 65536)
        v = FULL + (1024, 1024)
        _cycle(dev, plain(v, 300, "default", "counts+bytes"), plain(v, 300, "scan", "counts", window=(0, 0, 512, 512)))
        _cycle(dev, plain(v, 300, "default", "counts+bytes"), plain(v, 300, "group", "counts", times=3))


@pytest.mark.parametrize("kernel", ["default", "asm"])
@pytest.mark.parametrize("family", ["distance", "normals", "julia", "julia_distance"])
def test_two_pass_calls_and_julia(family, kernel):
    """Interposed: the two-pass form of the family on a ragged window without d_counts, through the stream's count scratch."""
    with MandelbrotDevice(0) as dev:
        if family == "distance":
            _cycle(dev, distance(*SEAHORSE, kernel), distance(*SEAHORSE, "default", window=RAGGED, with_counts=False))
        elif family == "normals":
            _cycle(dev, normals(*BLOCKS, kernel), normals(*BLOCKS, "group", window=RAGGED))
        elif family == "julia":
            _cycle(dev, julia(*JULIA, kernel), julia_distance(*JULIA, "default", window=RAGGED))
        else:
            _cycle(dev, julia_distance(*JULIA, kernel), julia_distance(*JULIA, "group", window=RAGGED))


@pytest.mark.parametrize("kernel", ["default", "group"])
def test_interior(kernel):
    with MandelbrotDevice(0) as dev:
        _cycle(dev, interior(*INTERIOR, kernel), interior(*INTERIOR, "scan", window=RAGGED))
        assert (interior(*INTERIOR, kernel).want(dev)["period"] > 0).sum() > 100


@pytest.mark.parametrize("kind,table", DEEP_KINDS, ids=[k + ("-table" if t else "") for k, t in DEEP_KINDS])
@pytest.mark.parametrize("family", ["deep", "wide"])
def test_deep_and_wide_views(family, kind, table):
    """Plain step and MBK_DEEP_BLA / MBK_DEEP_XBLA.  Interposed: the same call on the same orbit with a second dcmax -- the ctx
    keeps two tables beside an orbit, so nothing the graph reads is evicted."""
    orbit, view, view2, mrd = _deep() if family == "deep" else _wide()
    with MandelbrotDevice(0) as dev:
        _cycle(dev, deep(orbit, view, mrd, kind, table), deep(orbit, view2, mrd, kind, table, window=(3, 5, 40, 33)))
        assert len(np.unique(deep(orbit, view, mrd, kind, table).want(dev)["counts"])) > 1


@pytest.mark.parametrize("kind_of_view,what,s,threshold,rows", RENDERS,
                         ids=["-".join([k, w, f"s{s}"] + ([f"t{t}"] if w == "adaptive" else []) + (["bands"] if r else []))
                              for k, w, s, t, r in RENDERS])
def test_renders(kind_of_view, what, s, threshold, rows):
    """40 x 28 images.  Interposed: a smooth render of a window at s = 1 with the same palette, through the same render scratch."""
    pal = _render_palette()
    with MandelbrotDevice(0) as dev:
        lut = _lut(dev, kind_of_view) if what == "equalized" else None
        case = render(kind_of_view, what, pal, s=s, rows=rows, threshold=threshold, lut=lut)
        _cycle(dev, case, render(kind_of_view, "smooth", pal, s=1, window=(7, 5, 19, 13)))
        # the case is no flat image: the smooth colourings blend 53 entries over hundreds of values, a distance or a period
        # map holds the inside colour and a few entries at least; a threshold under 256 refines something
        want = case.want(dev)
        assert len(np.unique(want["rgba"])) > (3 if what in ("distance", "interior") else 50)
        if what == "adaptive":
            assert want["mask"].any() and (threshold > 0 or want["mask"].all())


def test_density_render():
    pal = _render_palette()
    view, target, mrd = DENSITY
    import torch
    with MandelbrotDevice(0) as dev:
        table = dev.compute_view_density(view, target, mrd)[0]
        d_table = torch.from_numpy(table.view(np.int32).copy()).to("cuda:0")
        assert table.max() > 3
        _cycle(dev, density_render(d_table, table, pal, "sqrt", 2), density_render(d_table, table, pal, "linear", 1))


@pytest.mark.parametrize("kind_of_view", ["plain", "julia", "deep", "wide"])
def test_histograms_accumulate_once_per_replay(kind_of_view):
    with MandelbrotDevice(0) as dev:
        _cycle_accumulate(dev, histogram(kind_of_view), histogram(kind_of_view, window=(3, 5, 40, 33)))


def test_density_accumulates_once_per_replay():
    with MandelbrotDevice(0) as dev:
        _cycle_accumulate(dev, density(None), density((3, 5, 30, 17)))


def test_counts_histogram():
    """mbk_counts_histogram: device pointers alone, no scratch -- capturable on a cold ctx."""
    import torch
    rng = np.random.RandomState(5)
    counts = rng.randint(0, 50, 5000).astype(np.int32)
    d_counts = torch.from_numpy(counts).to("cuda:0")
    with MandelbrotDevice(0) as dev:
        _cycle_accumulate(dev, counts_histogram(d_counts, counts, 5000, 50), counts_histogram(d_counts, counts, 1234, 50))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _small():
    """A launch that needs nothing of the ctx: capturable behind any refusal, on a cold ctx too."""
    return plain(SEAHORSE[0], SEAHORSE[1], "default", "counts")


def test_refused_on_a_cold_ctx():
    """No call has been made on the stream, no orbit has been used: every form that keeps scratch or reads an orbit copy is
    refused; a small plain launch, which needs neither, is captured behind the refusal."""
    pal = _render_palette()
    orbit, view, _, mrd = _deep()
    worbit, wview, _, _ = _wide()
    for bad, text in ((lambda dev: render("plain", "smooth", pal), "first call"),
                      (lambda dev: distance(*SEAHORSE, "default", with_counts=False), "first call"),
                      (lambda dev: plain(FULL + (1024, 1024), _ordered_mrd(dev), "group", "counts"), "first call"),
                      (lambda dev: deep(orbit, view, mrd, "counts", False), "reference orbit"),
                      (lambda dev: deep(worbit, wview, mrd, "distance", False), "reference orbit")):
        with MandelbrotDevice(0) as dev:
            _refusal(dev, bad(dev), _small(), text)


def test_refused_where_the_scratch_must_grow():
    pal = _render_palette()
    with MandelbrotDevice(0) as dev:
        # the count scratch of the two-pass forms: warm on a window, whole view inside the capture
        _refusal(dev, distance(*SEAHORSE, "default", with_counts=False), distance(*SEAHORSE, "default", window=RAGGED, with_counts=False),
                 "scratch must grow")
    with MandelbrotDevice(0) as dev:
        _refusal(dev, render("plain", "smooth", pal, s=3), render("plain", "smooth", pal, s=1), "scratch must grow")
    with MandelbrotDevice(0) as dev:
        # the dispatch lists: warm at 16 384 blocks, 16 512 inside the capture
        mrd = _ordered_mrd(dev)
        _refusal(dev, plain(FULL + (1032, 1024), mrd, "group", "counts"), plain(FULL + (1024, 1024), mrd, "group", "counts"),
                 "dispatch lists must grow")
    with MandelbrotDevice(0) as dev:
        # the units pre-pass' counters: the warm call took order 2, the captured one order 3
        mrd = _ordered_mrd(dev)
        dev.set_option("order", 2)
        case = plain(FULL + (1024, 1024), mrd, "group", "counts")

        def bad_launch(dev, o, s):
            dev.set_option("order", 3)
            dev.set_option("units_min_light", 0)
            try:
                case.launch(dev, o, s)
            finally:
                dev.set_option("order", 2)
        _refusal(dev, Case(case.outs, bad_launch, case.want), case, "units pre-pass")


def test_refused_with_another_palette_or_table():
    pal = _render_palette()
    other = Palette(pal.entries[::-1].copy(), inside=pal.inside, scale=pal.scale, offset=pal.offset)
    with MandelbrotDevice(0) as dev:
        _refusal(dev, render("plain", "smooth", other), render("plain", "smooth", pal), "palette differs")
    with MandelbrotDevice(0) as dev:
        lut = _lut(dev, "plain")
        lut2 = np.sqrt(lut)
        assert lut2.shape == lut.shape and (lut2 != lut).any() and lut2.min() >= 0.0 and lut2.max() <= 1.0
        _refusal(dev, render("plain", "equalized", pal, lut=lut2), render("plain", "equalized", pal, lut=lut), "equalisation table differs")
    with MandelbrotDevice(0) as dev:
        import torch
        table = np.arange(64 * 48, dtype=np.uint32).reshape(48, 64)
        d_table = torch.from_numpy(table.view(np.int32).copy()).to("cuda:0")

        def density(p):
            return Case(_image(64 * 48), lambda dev, o, s: dev.launch_render_density(d_table.data_ptr(), 64, 48, palette=p, d_rgba=o["rgba"].ptr, stream=s),
                        lambda dev: _rgba(dev.render_density(table, palette=p)[0]))
        _refusal(dev, density(other), density(pal), "palette differs")


def test_refused_without_a_resident_orbit_or_table():
    for family in ("deep", "wide"):
        orbit, view, view2, mrd = _deep() if family == "deep" else _wide()
        text = "table of this view's dcmax"
        with MandelbrotDevice(0) as dev:
            # a dcmax that is not resident: the warm call brought the other view's table
            _refusal(dev, deep(orbit, view2, mrd, "counts", True), deep(orbit, view, mrd, "counts", True), text)
        with MandelbrotDevice(0) as dev:
            _refusal(dev, deep(orbit, view2, mrd, "normals", True), deep(orbit, view, mrd, "distance", True), text)
        with MandelbrotDevice(0) as dev:
            # an orbit never used on the ctx
            _refusal(dev, deep(orbit, view, mrd, "nucleus", False), _small(), "reference orbit")
    with MandelbrotDevice(0) as dev:
        # the orbit's plain copy is there, its wide table is not
        orbit, view, _, mrd = _wide()
        plain_view = DeepView(1e-280, 64, 64)
        _refusal(dev, deep(orbit, view, mrd, "counts", False), deep(orbit, plain_view, mrd, "counts", False), "wide reference orbit")


@pytest.mark.parametrize("kernel", ["scan", "refill"])
def test_refused_selectors(kernel):
    """The two-pass "scan" alternates its cursor sets per enqueue and sizes its second pass from a hint the host reads; "refill"
    allocates its queues.  Both are refused inside a capture, through every call that takes a selector."""
    text = "MBK_KERNEL_" + kernel.upper()
    with MandelbrotDevice(0) as dev:
        _refusal(dev, plain(*SEAHORSE, kernel, "counts"), plain(*SEAHORSE, "group", "counts"), text)
    with MandelbrotDevice(0) as dev:
        big = FULL + (1024, 1024)
        _refusal(dev, plain(big, 300, kernel, "counts"), plain(big, 300, "default", "counts"), text)
    if kernel == "scan":
        pal = _render_palette()
        for bad, good in ((distance(*SEAHORSE, "scan", with_counts=False), distance(*SEAHORSE, "default", with_counts=False)),
                          (interior(*INTERIOR, "scan"), interior(*INTERIOR, "group")),
                          (render("plain", "smooth", pal, kernel="scan"), render("plain", "smooth", pal))):
            with MandelbrotDevice(0) as dev:
                _refusal(dev, bad, good, text)


def test_calls_that_cannot_be_captured():
    """The chunk launches read HOST input at enqueue time; mbk_density_max and mbk_reduce_counts wait for their result."""
    import torch
    from distributedmandelbrot_amd import _lib as L
    payload = np.random.RandomState(3).randint(0, 256, 4096).astype(np.uint8)
    raw = bytes([L.MBK_CODEC_RAW]) + payload.tobytes()
    one_run = bytes([L.MBK_CODEC_RLE]) + (L.MBK_CHUNK_BYTES).to_bytes(4, "little") + bytes([7])
    values = np.random.RandomState(4).randint(0, 1000, 3000).astype(np.int32)
    d_values = torch.from_numpy(values).to("cuda:0")
    results = {}

    def density_max(dev, o, s):
        results["max"] = dev.density_max(d_values.data_ptr(), values.size, stream=s)

    def reduce_counts(dev, o, s):
        results["reduce"] = dev.reduce_counts(d_values.data_ptr(), values.size, 1000, stream=s)
    cases = [
        (Case(lambda: {"bytes": Out("u1", 4096)}, lambda dev, o, s: dev.launch_decode_chunk(raw, d_bytes=o["bytes"].ptr, n=4096, hip_stream=s),
              lambda dev: {"bytes": payload}), "mbk_chunk_decode_launch"),
        (Case(_image(64 * 64), lambda dev, o, s: dev.launch_render_chunk(one_run, d_rgba=o["rgba"].ptr, scale=64, hip_stream=s),
              lambda dev: _rgba(dev.render_chunk(one_run, scale=64)[0])), "mbk_chunk_render_launch"),
        (Case(lambda: {}, density_max, lambda dev: {}), "mbk_density_max"),
        (Case(lambda: {}, reduce_counts, lambda dev: {}), "mbk_reduce_counts"),
    ]
    for bad, text in cases:
        with MandelbrotDevice(0) as dev:
            _refusal(dev, bad, _small(), text)
    assert results["max"] == (int(values.max()), int(values.sum()))
    st = results["reduce"]
    assert st.never_pixels == int((values == 0).sum()) and st.pixel_iterations == int(np.where(values > 0, values, 999).astype(np.int64).sum())
