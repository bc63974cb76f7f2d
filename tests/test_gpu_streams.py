"""Launch forms in flight on several streams of one context (include/mbk.h, "Streams"; DESIGN.md, "Streams").

A ctx keeps its helper state per stream (StreamScratch in csrc/mbk_api.hip: dispatch lists with their pre-pass stream and events,
scan cursors, spill buffers, render and count scratch, palette, equalisation table, density band words, XCD share ring) and guards
what it keeps once -- orbit copies, the two table places beside an orbit, the scratch table itself -- by draining the device.
Every other GPU file issues a launch on one stream and waits.  A wrong sharing of per-stream state gives wrong pixels only where
two launches overlap, and a missing drain only where a reader is still queued: this file arranges both.

Expected values are the bits of the synchronous forms (want(dev) of a catalogue case, tests/launch_cases.py), computed on a
SECOND MandelbrotDevice and compared byte for byte, guards included; the other GPU files hold those bits to models and truth.

In flight.  The cases are milliseconds of work and would end before the next is enqueued.  So every stream first gets a ballast
that is not the library's -- torch.cuda._sleep for BALLAST_MS, with an event behind it -- and the launches queue behind it and
start together when it ends.  Every test that claims overlap asserts it: right after the last enqueue (or right before a call
that is expected to wait) the ballasts' events must still be pending.  profiles/streams/README.md has the measured enqueue times
that BALLAST_MS rests on.
"""
import ctypes
import random
import time
from dataclasses import dataclass

import numpy as np
import pytest

import deep_adaptive_cases as K
import deep_bla_model as B
import deep_wide_adaptive_cases as KW
import deep_wide_bla_model as X
from distributedmandelbrot_amd import DeepOrbit, DeepView, MandelbrotDevice, Palette, WideDeepView
from launch_cases import (BLOCKS, DEEP_KINDS, DENSITY, FULL, INTERIOR, JULIA, RAGGED, RENDERS, SEAHORSE, Case, _check, _deep, _image, _lut,
                          _ordered_mrd, _render_palette, _rgba, _wide, counts_histogram, deep, density, density_render, distance, histogram,
                          interior, julia, julia_distance, normals, plain, render)

pytestmark = pytest.mark.gpu

# The longest enqueue sequence of the file -- twelve ballasts and the 71 forms of a round of test_every_form_beside_the_others --
# takes the host 1.02 to 1.43 ms (profiles/streams/README.md); every other sequence is under 0.5 ms.  Four times the longest is
# 5.7 ms -- host time varies by that much on a box that others share -- and the round figure above it costs the file nothing.
BALLAST_MS = 10.0

_CACHE = {}


def _cycles_per_ms(torch) -> float:
    """What torch.cuda._sleep counts, per millisecond: measured once with events, on a sleep of 5 ms at least."""
    if "rate" not in _CACHE:
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
                break
            n *= 10
        _CACHE["rate"] = n / ms
        print("ballast: %d cycles of torch.cuda._sleep took %.2f ms" % (n, ms))
    return _CACHE["rate"]


class Ballast:
    """BALLAST_MS of sleep on each of `streams` (torch streams), and behind each an event."""

    def __init__(self, torch, streams, ms: float = BALLAST_MS):
        cycles = int(_cycles_per_ms(torch) * ms)
        self.events = []
        self.t0 = time.perf_counter()      # the first ballast runs while the others are enqueued
        for s in streams:
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
            e = torch.cuda.Event()
            e.record(s)
            self.events.append(e)

    def pending(self):
        return [not e.query() for e in self.events]

    def assert_in_flight(self, what):
        p = self.pending()
        print("%.2f ms from the first ballast's enqueue, %d ballasts, %d still pending: %s" % ((time.perf_counter() - self.t0) * 1e3, len(p), sum(p), what))
        assert all(p), (what, "a ballast ended before this point: nothing proves that the launches overlap", p)


def _streams(torch, n):
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(n)]
    assert len({s.cuda_stream for s in streams}) == n and all(s.cuda_stream != 0 for s in streams)
    return streams


def _fresh(torch, *groups):
    """Sentinels in every output (zeros in the body of an accumulating one), then a device sync: fill_ runs on torch's stream."""
    for outs, accumulate in groups:
        for o in outs.values():
            o.refill()
            if accumulate:
                o.zero_body()
    torch.cuda.synchronize()


def _other_palette(pal):
    return Palette(pal.entries[::-1].copy(), inside=pal.inside, scale=pal.scale, offset=pal.offset)


@dataclass
class Form:
    name: str
    case: Case
    want: dict               # what the synchronous form stores, computed once on a device of its own and left unchanged
    accumulate: bool = False


def _catalogue():
    """One case per launch form, with its expected bits.  The four equalised renders come first: each carries a table of its
    own, a stream keeps one table, and a render with another waits for its stream -- dealt round-robin over 4 or 12 streams
    they land on four different ones.  The extended-range kinds run at 40 x 28, the renders' shape: with the fine view of the
    adaptive render at s = 3 that makes two dcmax on the orbit, which is what a ctx keeps (a third would drain the device on
    every launch, by design); the deep kinds at 64 x 64 are the deep orbit's second dcmax beside the renders' one."""
    if "forms" in _CACHE:
        return _CACHE["forms"]
    import torch
    pal = _render_palette()
    forms = []
    with MandelbrotDevice(0) as ref:
        def add(name, case, accumulate=False):
            forms.append(Form(name, case, case.want(ref), accumulate))
        for k in ("plain", "deep", "wide", "julia"):
            add(f"render-{k}-equalized", render(k, "equalized", pal, lut=_lut(ref, k)))
        for kernel in ("default", "group", "asm", "scan"):
            for outputs in ("counts", "bytes", "smooth"):
                add(f"plain-{kernel}-{outputs}", plain(*SEAHORSE, kernel, outputs))
        add("distance-counts", distance(*SEAHORSE, "default"))
        add("distance", distance(*SEAHORSE, "default", with_counts=False))
        add("normals", normals(*BLOCKS, "default"))
        add("interior", interior(*INTERIOR, "default"))
        add("julia", julia(*JULIA, "default"))
        add("julia-distance", julia_distance(*JULIA, "default"))
        for family in ("deep", "wide"):
            orbit, view, _, mrd = _deep() if family == "deep" else _wide(40, 28)
            for kind, table in DEEP_KINDS:
                add(f"{family}-{kind}" + ("-table" if table else ""), deep(orbit, view, mrd, kind, table))
        for k, w, s, t, rows in RENDERS:
            if w != "equalized":
                add("-".join(["render", k, w, f"s{s}", f"t{t}"] + (["bands"] if rows else [])), render(k, w, pal, s=s, rows=rows, threshold=t))
        view, target, mrd = DENSITY
        table = ref.compute_view_density(view, target, mrd)[0]
        d_table = torch.from_numpy(table.view(np.int32).copy()).to("cuda:0")
        add("density-render", density_render(d_table, table, pal, "sqrt", 2))
        counts = np.random.RandomState(5).randint(0, 50, 5000).astype(np.int32)
        add("counts-histogram", counts_histogram(torch.from_numpy(counts).to("cuda:0"), counts, 5000, 50), accumulate=True)
    assert len({f.name for f in forms}) == len(forms)
    # two dcmax per orbit, no more: the views that take a table, by the models' dcmax
    deep_views = [DeepView(1e-12, 64, 64)] + [K.finer(DeepView(1e-12, 40, 28), s) for s in (1, 2, 3)]
    wide_views = [KW.finer(WideDeepView(1.0, -1100, 40, 28), s) for s in (1, 2, 3)]
    assert len({float(B.dcmax(v)) for v in deep_views}) <= 2 and len({X.dcmax(v) for v in wide_views}) <= 2
    _CACHE["forms"] = forms
    return forms


def _by_name(name):
    return next(f for f in _catalogue() if f.name == name)


# ---- 1, 2: every form beside the others, warm ------------------------------------------------------------------------------------

def _every_form(devs, n_streams):
    import torch
    forms = _catalogue()
    streams = _streams(torch, n_streams)
    n = len(forms)
    outs = [f.case.outs() for f in forms]
    where = [(devs[(i % n_streams) % len(devs)], streams[i % n_streams]) for i in range(n)]
    _fresh(torch, *[(o, f.accumulate) for o, f in zip(outs, forms)])
    try:
        for f, o, (dev, s) in zip(forms, outs, where):      # every (form, stream) pair once, with a sync
            f.case.launch(dev, o, s.cuda_stream)
            s.synchronize()
            _check(o, f.want, ("warm call", f.name))
        _fresh(torch, *[(o, f.accumulate) for o, f in zip(outs, forms)])
        order = list(range(n))
        for rnd in range(3):
            if rnd == 1:
                order = order[n // 3:] + order[:n // 3]
            elif rnd == 2:
                random.Random(7).shuffle(order)
            ballast = Ballast(torch, streams)
            for i in order:
                forms[i].case.launch(where[i][0], outs[i], where[i][1].cuda_stream)
            ballast.assert_in_flight(("round", rnd, n, "launches"))        # warm launch forms wait for nothing (mbk.h)
    finally:
        torch.cuda.synchronize()
    for f, o in zip(forms, outs):
        _check(o, f.want, f.name, factor=3 if f.accumulate else 1)


@pytest.mark.parametrize("n_streams", [4, 12])
def test_every_form_beside_the_others(n_streams):
    """71 forms dealt round-robin over the streams of one ctx, three rounds back to back behind fresh ballasts, each in another
    order, with no synchronisation by the test between launches; then one device sync and every output and guard."""
    with MandelbrotDevice(0) as dev:
        _every_form([dev], n_streams)


@pytest.mark.parametrize("n_streams", [4, 12])
def test_every_form_on_two_contexts(n_streams):
    """The same with the streams alternating between two ctxs of the GPU that share the deep and the wide orbit (mbk.h: an orbit
    may be used by any number of ctxs)."""
    with MandelbrotDevice(0) as one, MandelbrotDevice(0) as two:
        _every_form([one, two], n_streams)


# ---- 3: cold beside warm ------------------------------------------------------------------------------------------------------------

def test_cold_calls_beside_a_warm_stream():
    """Stream A is warm and has a render, a two-pass distance, an ordered launch and a table launch queued behind a ballast each
    time stream B makes its FIRST call of a kind: a render (palette upload, scratch), a two-pass distance without d_counts, an
    ordered launch (auxiliary stream, lists, events), a table launch of a new dcmax into the orbit's free place."""
    import torch
    pal = _render_palette()
    orbit, view, view2, dmrd = _deep()
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        mrd = _ordered_mrd(dev)
        assert mrd == _ordered_mrd(ref)
        warm = [render("plain", "smooth", pal), distance(*SEAHORSE, "default", with_counts=False),
                plain(FULL + (1024, 1024), mrd, "group", "counts"), deep(orbit, view, dmrd, "counts", True)]
        cold = [render("plain", "relief", pal, s=3), distance(*BLOCKS, "default", with_counts=False),
                plain(FULL + (2048, 2048), mrd, "group", "counts", window=(512, 512, 1024, 1024)), deep(orbit, view2, dmrd, "counts", True)]
        wwant, cwant = [c.want(ref) for c in warm], [c.want(ref) for c in cold]
        a, b = _streams(torch, 2)
        wouts, couts = [c.outs() for c in warm], [c.outs() for c in cold]
        _fresh(torch, *[(o, False) for o in wouts + couts])
        try:
            for c, o, w in zip(warm, wouts, wwant):
                c.launch(dev, o, a.cuda_stream)
                a.synchronize()
                _check(o, w, "warm call on A")
            _fresh(torch, *[(o, False) for o in wouts])
            for k, c in enumerate(cold):
                ballast = Ballast(torch, [a])
                for w, o in zip(warm, wouts):
                    w.launch(dev, o, a.cuda_stream)
                ballast.assert_in_flight(("A is queued before the cold call", k))
                c.launch(dev, couts[k], b.cuda_stream)
                print("cold call %d on B: A's ballast still pending afterwards: %s" % (k, ballast.pending()[0]))
        finally:
            torch.cuda.synchronize()
        for o, w in zip(wouts, wwant):
            _check(o, w, "A")
        for o, w in zip(couts, cwant):
            _check(o, w, "B, cold")


# ---- 4: scratch growth behind queued work ----------------------------------------------------------------------------------------

def test_scratch_growth_behind_queued_work():
    """On stream A behind a ballast: a render at s = 1, then at s = 3 (the render scratch grows); a two-pass distance on a
    ragged window, then on the whole view (the count scratch grows); an ordered launch of 16 384 blocks, then of 16 512 (the
    dispatch lists grow).  The old buffer of each may be freed only behind the smaller launch that is still queued.  Stream B
    has renders and ordered launches queued behind its own ballast throughout."""
    import torch
    pal = _render_palette()
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        mrd = _ordered_mrd(dev)
        pairs = [(render("plain", "smooth", pal, s=1), render("plain", "smooth", pal, s=3)),
                 (distance(*SEAHORSE, "default", window=RAGGED, with_counts=False), distance(*SEAHORSE, "default", with_counts=False)),
                 (plain(FULL + (1024, 1024), mrd, "group", "counts"), plain(FULL + (1032, 1024), mrd, "group", "counts"))]
        beside = [render("plain", "relief", pal, s=2), plain(FULL + (2048, 2048), mrd, "group", "counts", window=(512, 512, 1024, 1024))]
        pwant = [(small.want(ref), big.want(ref)) for small, big in pairs]
        bwant = [c.want(ref) for c in beside]
        a, b = _streams(torch, 2)
        pouts = [(small.outs(), big.outs()) for small, big in pairs]
        bouts = [c.outs() for c in beside]
        everything = [(o, False) for pair in pouts for o in pair] + [(o, False) for o in bouts]
        _fresh(torch, *everything)
        try:
            for (small, _), (o, _), (w, _) in zip(pairs, pouts, pwant):     # A has seen the smaller need of each kind, B its own
                small.launch(dev, o, a.cuda_stream)
                a.synchronize()
                _check(o, w, "warm call on A")
            for c, o, w in zip(beside, bouts, bwant):
                c.launch(dev, o, b.cuda_stream)
                b.synchronize()
                _check(o, w, "warm call on B")
            _fresh(torch, *everything)
            for k, ((small, big), (so, bo)) in enumerate(zip(pairs, pouts)):
                ballast = Ballast(torch, [b, a])
                for c, o in zip(beside, bouts):
                    c.launch(dev, o, b.cuda_stream)
                small.launch(dev, so, a.cuda_stream)
                ballast.assert_in_flight(("before the launch that grows the scratch", k))
                big.launch(dev, bo, a.cuda_stream)
                print("growth %d: ballasts pending afterwards (B, A): %s" % (k, ballast.pending()))
        finally:
            torch.cuda.synchronize()
        for (so, bo), (sw, bw) in zip(pouts, pwant):
            _check(so, sw, "A, the smaller launch")
            _check(bo, bw, "A, the launch that grew the scratch")
        for o, w in zip(bouts, bwant):
            _check(o, w, "B")


# ---- 5: palette and table changes -------------------------------------------------------------------------------------------------

def _palette_cases(ref, pal, lut):
    """(smooth render, equalised render, density render) with the palette pal and the table lut, and what each stores."""
    import torch
    view, target, mrd = DENSITY
    if "density" not in _CACHE:
        table = ref.compute_view_density(view, target, mrd)[0]
        _CACHE["density"] = (table, torch.from_numpy(table.view(np.int32).copy()).to("cuda:0"))
    table, d_table = _CACHE["density"]
    cases = [render("plain", "smooth", pal), render("plain", "equalized", pal, lut=lut), density_render(d_table, table, pal, "sqrt", 1)]
    return cases, [c.want(ref) for c in cases]


def test_each_stream_keeps_its_own_palette_and_table():
    """Two streams, two palettes, two equalisation tables: stream A renders with (P, lut), stream B with (Q, lut2), alternating
    behind ballasts.  Each stream's device copies stay what its last render uploaded, so nothing waits, and each image is its own
    palette's and table's."""
    import torch
    pal = _render_palette()
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        lut = _lut(ref, "plain")
        mine, mwant = _palette_cases(ref, pal, lut)
        theirs, twant = _palette_cases(ref, _other_palette(pal), np.sqrt(lut))
        for w, v in zip(mwant, twant):
            assert (w["rgba"] != v["rgba"]).mean() > 0.1         # the two palettes (and tables) give different images
        a, b = _streams(torch, 2)
        rounds = 2
        mouts = [[c.outs() for c in mine] for _ in range(rounds)]
        touts = [[c.outs() for c in theirs] for _ in range(rounds)]
        everything = [(o, False) for group in mouts + touts for o in group]
        _fresh(torch, *everything)
        try:
            for c, o in zip(mine, mouts[0]):
                c.launch(dev, o, a.cuda_stream)
            for c, o in zip(theirs, touts[0]):
                c.launch(dev, o, b.cuda_stream)
            torch.cuda.synchronize()
            for o, w in zip(mouts[0] + touts[0], mwant + twant):
                _check(o, w, "warm call")
            _fresh(torch, *everything)
            ballast = Ballast(torch, [a, b])
            for r in range(rounds):
                for k in range(len(mine)):
                    mine[k].launch(dev, mouts[r][k], a.cuda_stream)
                    theirs[k].launch(dev, touts[r][k], b.cuda_stream)
            ballast.assert_in_flight("nothing waits while each stream keeps its palette and table")
        finally:
            torch.cuda.synchronize()
        for r in range(rounds):
            for o, w in zip(mouts[r] + touts[r], mwant + twant):
                _check(o, w, ("round", r))


@pytest.mark.parametrize("what", ["palette", "table", "density-palette"])
def test_a_change_waits_for_the_renders_that_read_the_old_one(what):
    """One stream: a render with palette P (table lut) queued behind a ballast, then at once the same with palette Q (table lut2):
    the device copy is overwritten in place, so the library must wait for the first render.  Both images are right.  A second
    stream with a ballast of its own shows that the first render was still queued when the second call came."""
    import torch
    pal = _render_palette()
    k = {"palette": 0, "table": 1, "density-palette": 2}[what]
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        lut = _lut(ref, "plain")
        first, fwant = _palette_cases(ref, pal, lut)
        second, swant = _palette_cases(ref, _other_palette(pal) if what != "table" else pal, np.sqrt(lut))
        first, fwant, second, swant = first[k], fwant[k], second[k], swant[k]
        assert (fwant["rgba"] != swant["rgba"]).mean() > 0.1
        s, other = _streams(torch, 2)
        fo, so, fo2 = first.outs(), second.outs(), first.outs()
        _fresh(torch, (fo, False), (so, False), (fo2, False))
        try:
            first.launch(dev, fo, s.cuda_stream)
            s.synchronize()
            _check(fo, fwant, "warm call")
            _fresh(torch, (fo, False))
            ballast = Ballast(torch, [s, other])
            first.launch(dev, fo, s.cuda_stream)
            ballast.assert_in_flight("the first render is queued when the second call comes")
            second.launch(dev, so, s.cuda_stream)
            first.launch(dev, fo2, s.cuda_stream)        # and back, behind the second one
        finally:
            torch.cuda.synchronize()
        _check(fo, fwant, "the render before the change")
        _check(so, swant, "the render with the new " + what)
        _check(fo2, fwant, "back to the first " + what)


# ---- 6: table places under readers --------------------------------------------------------------------------------------------------

def _adaptive(orbit, view, mrd, pal, s, threshold) -> Case:
    """An adaptive render with a table, of a view whose base and fine dcmax differ: it needs both places of the orbit at once."""
    wide = isinstance(view, WideDeepView)
    name = "render_wide_view_adaptive" if wide else "render_deep_view_adaptive"
    flag = {"xbla": True} if wide else {"bla": True}
    common = dict(palette=pal, supersample=s, threshold=threshold)

    def want(dev):
        img, mask, _ = getattr(dev, name)(orbit, view, mrd, want_mask=True, **common, **flag)
        return dict(_rgba(img), mask=mask)
    return Case(_image(view.width * view.height, mask=True),
                lambda dev, o, st: getattr(dev, "launch_" + name)(orbit, view, mrd, d_rgba=o["rgba"].ptr, d_mask=o["mask"].ptr, stream=st,
                                                                  **common, **flag), want)


def _three_views(family):
    if family == "deep":
        orbit, v1, v2, mrd = _deep()
        return orbit, (v1, v2, DeepView(4e-12, 64, 64)), mrd
    orbit, v1, v2, mrd = _wide()
    return orbit, (v1, v2, WideDeepView(1.0, -1098, 64, 64)), mrd


@pytest.mark.parametrize("kind", ["counts", "distance", "normals"])
@pytest.mark.parametrize("family", ["deep", "wide"])
def test_a_table_place_is_evicted_under_a_reader_on_another_stream(family, kind):
    """One orbit, three dcmax, two places (MBK_DEEP_BLA / MBK_DEEP_XBLA).  With the tables of views 2 and 3 resident: A has view 3
    queued behind a ballast, B view 2; then B launches view 1, whose table goes over the one asked for least recently -- view 3's,
    which A's queued launch reads.  Again with views 2 and 1 resident: A view 1, B view 2, then B view 3 over view 1's table.
    The library drains the device before it overwrites a place; every output is its own view's.  (The readers are warm: an orbit's
    upload and a table's first build are synchronous copies, and whether the runtime waits for queued work inside one is not
    the library's to say -- profiles/streams/README.md.  test_cold_calls_beside_a_warm_stream has the cold table.)"""
    import torch
    orbit, views, mrd = _three_views(family)
    cases = [deep(orbit, v, mrd, kind, True) for v in views]
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        want = [c.want(ref) for c in cases]
        assert len({w["counts"].tobytes() for w in want}) == 3
        a, b = _streams(torch, 2)
        steps = [(a, 2), (b, 1), (b, 0), (a, 0), (b, 1), (b, 2)]       # (stream, view): the third and the sixth evict
        outs = [cases[v].outs() for _, v in steps]
        wouts = [c.outs() for c in cases]
        _fresh(torch, *[(o, False) for o in outs + wouts])
        try:
            for (s, v) in ((a, 0), (b, 1), (a, 2)):                      # both streams warm; views 2 and 3 resident, 3 the later
                cases[v].launch(dev, wouts[v], s.cuda_stream)
                s.synchronize()
                _check(wouts[v], want[v], "warm call")
            for half in (0, 3):
                ballast = Ballast(torch, [a, b])
                for k in (half, half + 1):
                    s, v = steps[k]
                    cases[v].launch(dev, outs[k], s.cuda_stream)
                ballast.assert_in_flight(("readers are queued before the eviction", half))
                s, v = steps[half + 2]
                cases[v].launch(dev, outs[half + 2], s.cuda_stream)
        finally:
            torch.cuda.synchronize()
        for k, (_, v) in enumerate(steps):
            _check(outs[k], want[v], ("step", k, "view", v))


@pytest.mark.parametrize("family", ["deep", "wide"])
def test_both_tables_of_an_adaptive_render_under_a_third_dcmax(family):
    """Stream A renders adaptively a view whose base and fine dcmax differ: both places of the orbit.  Stream B holds a third
    dcmax.  B's launch is queued behind a ballast when A's render evicts its table, and A's render when B's launch evicts one of
    its two."""
    import torch
    if family == "deep":
        orbit, view, mrd, pal, mid = K.case("i-30-two-tables")
        assert B.dcmax(view) != B.dcmax(K.finer(view, 2))
        third = DeepView(2e-30, view.width, view.height)
        assert B.dcmax(third) not in (B.dcmax(view), B.dcmax(K.finer(view, 2)))
    else:
        orbit, view, mrd, pal, mid = KW.case("i-1100-two-tables")
        assert X.dcmax(view) != X.dcmax(KW.finer(view, 2))
        third = WideDeepView(1.0, -1099, view.width, view.height)
        assert X.dcmax(third) not in (X.dcmax(view), X.dcmax(KW.finer(view, 2)))
    ca, cb = _adaptive(orbit, view, mrd, pal, 2, mid), deep(orbit, third, mrd, "counts", True)
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        wa, wb = ca.want(ref), cb.want(ref)
        assert 0 < int(wa["mask"].sum()) < wa["mask"].size
        a, b = _streams(torch, 2)
        oa, ob = [ca.outs() for _ in range(3)], [cb.outs() for _ in range(3)]
        _fresh(torch, *[(o, False) for o in oa + ob])
        try:
            ca.launch(dev, oa[0], a.cuda_stream)        # warm: palette, scratch, both tables; then B's over one of them
            a.synchronize()
            cb.launch(dev, ob[0], b.cuda_stream)
            b.synchronize()
            ballast = Ballast(torch, [a, b])
            cb.launch(dev, ob[1], b.cuda_stream)
            ballast.assert_in_flight("B's launch is queued before A's render evicts its table")
            ca.launch(dev, oa[1], a.cuda_stream)
            ballast = Ballast(torch, [a, b])
            ca.launch(dev, oa[2], a.cuda_stream)
            ballast.assert_in_flight("A's render is queued before B's launch evicts one of its tables")
            cb.launch(dev, ob[2], b.cuda_stream)
        finally:
            torch.cuda.synchronize()
        for o in oa:
            _check(o, wa, "A, adaptive")
        for o in ob:
            _check(o, wb, "B, third dcmax")


# ---- 7: orbit copies under readers ----------------------------------------------------------------------------------------------------

def test_orbit_copies_are_dropped_under_readers_on_caller_streams():
    """Eight orbits are resident (all a ctx keeps).  Launches of three of them are queued behind ballasts on three caller streams
    when a ninth orbit, on a fourth stream, makes the ctx drop every copy -- behind a drain.  Every result is its own orbit's,
    and so is a launch of an evicted orbit afterwards.  Orbits of equal length whose pictures differ, as in tests/test_gpu_deep.py."""
    import torch
    mrd = 3000
    orbits = [DeepOrbit("%.20f" % (0.25 - k * 2.0 ** -19), "0", mrd, min_span=1e-30) for k in range(9)]
    view = DeepView(1e-4, 48, 8, 1e-30)
    cases = [deep(o, view, mrd, "counts", False) for o in orbits]
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        want = [c.want(ref) for c in cases]
        assert len({w["counts"].tobytes() for w in want}) == 9
        streams = _streams(torch, 4)
        outs = [c.outs() for c in cases]
        again = {k: cases[k].outs() for k in (5, 0)}
        _fresh(torch, *[(o, False) for o in outs + list(again.values())])
        try:
            for k in range(8):
                cases[k].launch(dev, outs[k], streams[k % 3].cuda_stream)
            torch.cuda.synchronize()
            for k in range(8):
                _check(outs[k], want[k], ("resident", k))
            _fresh(torch, *[(o, False) for o in outs])
            ballast = Ballast(torch, streams[:3])
            for s, k in zip(streams[:3], (5, 6, 7)):
                cases[k].launch(dev, outs[k], s.cuda_stream)
            ballast.assert_in_flight("three readers are queued before the ninth orbit comes")
            cases[8].launch(dev, outs[8], streams[3].cuda_stream)
            for k in (5, 0):
                cases[k].launch(dev, again[k], streams[3].cuda_stream)
        finally:
            torch.cuda.synchronize()
        for k in (5, 6, 7, 8):
            _check(outs[k], want[k], ("orbit", k))
        for k in (5, 0):
            _check(again[k], want[k], ("evicted and used again", k))


# ---- 8: accumulating forms into one table ---------------------------------------------------------------------------------------------

def _tiles(w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return [(0, 0, cw, ch), (cw, 0, w - cw, ch), (0, ch, cw, h - ch), (cw, ch, w - cw, h - ch)]


@pytest.mark.parametrize("what", ["histogram", "density"])
def test_four_streams_add_into_one_table(what):
    """Four streams add into the SAME device table behind ballasts: the four windows that tile the view twice each, one per
    stream, then the whole view from every stream.  The table is the sum of the synchronous forms' tables of what was launched."""
    import torch
    if what == "histogram":
        make, key, (w, h) = (lambda window: histogram("plain", window)), "hist", SEAHORSE[0][4:6]
    else:
        make, key, (w, h) = density, "table", (DENSITY[0].width, DENSITY[0].height)
    windows = _tiles(w, h)
    cases, whole = [make(win) for win in windows], make(None)
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        wants = [c.want(ref)[key] for c in cases]
        wwant = whole.want(ref)[key]
        total = sum(2 * x.astype(np.int64) for x in wants) + 4 * wwant.astype(np.int64)
        assert wwant.any() and all(x.any() for x in wants)
        streams = _streams(torch, 4)
        table, scrap = whole.outs(), whole.outs()
        _fresh(torch, (table, True), (scrap, True))
        try:
            for s in streams:                         # each stream's sample scratch at its largest
                whole.launch(dev, scrap, s.cuda_stream)
            torch.cuda.synchronize()
            _check(scrap, {key: wwant}, "warm calls", factor=4)
            ballast = Ballast(torch, streams)
            for _ in range(2):
                for s, c in zip(streams, cases):
                    c.launch(dev, table, s.cuda_stream)
            for s in streams:
                whole.launch(dev, table, s.cuda_stream)
            ballast.assert_in_flight("twelve launches into one table are queued")
        finally:
            torch.cuda.synchronize()
        _check(table, {key: total.astype(wwant.dtype)}, what)


# ---- 9: the ordered path across streams -------------------------------------------------------------------------------------------------

ORDERS = [(2, 0), (3, 0), (3, 1)]


@pytest.mark.parametrize("cycle_detect", [0, 1])
@pytest.mark.parametrize("order,xcd_balance", ORDERS, ids=["order2", "units", "units-balance"])
@pytest.mark.parametrize("prepass_overlap", [0, 1, 2])
def test_ordered_launches_across_streams(prepass_overlap, order, xcd_balance, cycle_detect):
    """Three streams, four ordered launches each (16 384 blocks: a pre-pass into a list of the stream's ring, on the stream's
    auxiliary stream under prepass_overlap 1 / 2, and the tile kernel), enqueued alternating between the streams behind
    ballasts: every ring, every auxiliary stream and every event belongs to one stream.  Then prepass_overlap changes and each
    stream runs once more: the first launch of the new mode drains its two streams."""
    import torch
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        for d in (ref, dev):
            d.set_option("prepass_overlap", prepass_overlap)
            d.set_option("cycle_detect", cycle_detect)
            d.set_option("order", order)
            if order == 3:
                d.set_option("units_min_light", 0)
                d.set_option("xcd_balance", xcd_balance)
        mrd = _ordered_mrd(dev)
        two = [plain(FULL + (1024, 1024), mrd, "group", "counts"),
               plain(FULL + (2048, 2048), mrd, "group", "counts", window=(512, 512, 1024, 1024))]
        want = [c.want(ref) for c in two]
        assert len(np.unique(want[0]["counts"])) > 10 and want[0]["counts"].tobytes() != want[1]["counts"].tobytes()
        streams = _streams(torch, 3)
        outs = [[two[k % 2].outs() for k in range(4)] for _ in streams]
        later = [two[1].outs() for _ in streams]
        everything = [(o, False) for group in outs + [later] for o in group]
        _fresh(torch, *everything)
        try:
            for s, group in zip(streams, outs):
                two[0].launch(dev, group[0], s.cuda_stream)
                s.synchronize()
                _check(group[0], want[0], "warm call")
            _fresh(torch, *everything)
            ballast = Ballast(torch, streams)
            for k in range(4):
                for s, group in zip(streams, outs):
                    two[k % 2].launch(dev, group[k], s.cuda_stream)
            ballast.assert_in_flight("twelve ordered launches are queued")
            torch.cuda.synchronize()
            for group in outs:
                for k in range(4):
                    _check(group[k], want[k % 2], ("launch", k))
            _fresh(torch, *everything)
            ballast = Ballast(torch, streams)
            for s, group in zip(streams, outs):
                two[1].launch(dev, group[1], s.cuda_stream)      # the old mode still: queued
            ballast.assert_in_flight("launches of the old mode are queued before the first of the new one")
            dev.set_option("prepass_overlap", (prepass_overlap + 1) % 3)
            for s, group, o in zip(streams, outs, later):
                two[0].launch(dev, group[0], s.cuda_stream)      # the first of the new mode on this stream: drains it
                two[1].launch(dev, o, s.cuda_stream)
        finally:
            torch.cuda.synchronize()
        for group, o in zip(outs, later):
            _check(group[1], want[1], "the last launch of the old mode")
            _check(group[0], want[0], "the first launch of the new mode")
            _check(o, want[1], "the second launch of the new mode")


# ---- 10: synchronous forms beside launches ----------------------------------------------------------------------------------------------

def test_synchronous_forms_beside_queued_launches():
    """Launch forms are queued behind ballasts on three caller streams while the same ctx runs synchronous forms on its own
    streams and buffers: smooth values, a render, a histogram, a deep view with a table, an adaptive render.  Both sides are right."""
    import torch
    names = ["plain-default-smooth", "render-plain-smooth-s2-t0", "deep-counts-table", "render-plain-adaptive-s2-t16", "render-deep-relief-s2-t0",
             "distance", "plain-scan-counts"]
    queued = [_by_name(n) for n in names]
    hist = histogram("plain")
    with MandelbrotDevice(0) as ref, MandelbrotDevice(0) as dev:
        hwant = hist.want(ref)
        streams = _streams(torch, 3)
        outs = [f.case.outs() for f in queued]
        _fresh(torch, *[(o, False) for o in outs])
        try:
            for k, (f, o) in enumerate(zip(queued, outs)):
                f.case.launch(dev, o, streams[k % 3].cuda_stream)
            torch.cuda.synchronize()
            for f, o in zip(queued, outs):
                _check(o, f.want, ("warm call", f.name))
            _fresh(torch, *[(o, False) for o in outs])
            ballast = Ballast(torch, streams)
            for k, (f, o) in enumerate(zip(queued, outs)):
                f.case.launch(dev, o, streams[k % 3].cuda_stream)
            ballast.assert_in_flight("launches are queued before the synchronous calls")
            got = []
            for f in queued[:4] + [Form("histogram", hist, hwant)]:
                got.append(f.case.want(dev))
                print("ballasts pending after the synchronous form of %s: %s" % (f.name, ballast.pending()))
        finally:
            torch.cuda.synchronize()
        for f, g in zip(queued[:4] + [Form("histogram", hist, hwant)], got):
            assert set(g) == set(f.want), f.name
            for key in g:
                assert np.ascontiguousarray(g[key]).tobytes() == np.ascontiguousarray(f.want[key]).tobytes(), (f.name, key)
        for f, o in zip(queued, outs):
            _check(o, f.want, f.name)


# ---- 11: more than 64 streams ------------------------------------------------------------------------------------------------------------

def _hip_runtime():
    """The HIP runtime this process has loaded (distributedmandelbrot_amd/_lib.py decides which copy that is)."""
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths.pop())
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamCreateWithFlags.restype = ctypes.c_int
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    hip.hipStreamDestroy.restype = ctypes.c_int
    return hip


def test_more_streams_than_the_scratch_table_holds():
    """66 distinct streams, each with a small render and a two-pass distance of its own, with no sync by the test: on the 65th the
    ctx drains the device and drops the scratch of all 64.  Then streams 1 to 3 again -- their scratch is made anew, the palette
    uploaded again -- and stream 1 with another palette.  Every output is right.  (No ballast: 130 launches with their
    allocations take the host far longer than the work takes the device.)"""
    import torch
    pal = _render_palette()
    forms = [_by_name("render-plain-smooth-s2-t0"), _by_name("distance")]
    other = render("plain", "smooth", _other_palette(pal))
    keep, handles, made = [], [], []
    for priority in (0, -1):                       # torch hands out a fixed number of pool streams per priority, in turn
        for _ in range(40):
            s = torch.cuda.Stream(device="cuda:0", priority=priority)
            if s.cuda_stream != 0 and s.cuda_stream not in handles and len(handles) < 66:
                keep.append(s)
                handles.append(s.cuda_stream)
    hip = _hip_runtime() if len(handles) < 66 else None
    print("distinct torch streams: %d of 66" % len(handles))
    try:
        while len(handles) < 66:
            h = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0      # hipStreamNonBlocking
            assert h.value and h.value not in handles
            made.append(h.value)
            handles.append(h.value)
        assert len(set(handles)) == 66
        with MandelbrotDevice(0) as ref:
            owant = other.want(ref)
        with MandelbrotDevice(0) as dev:
            outs = [[f.case.outs() for f in forms] for _ in handles]
            again = [[f.case.outs() for f in forms] for _ in range(3)]
            oo = other.outs()
            _fresh(torch, *[(o, False) for group in outs + again for o in group], (oo, False))
            try:
                for h, group in zip(handles, outs):
                    for f, o in zip(forms, group):
                        f.case.launch(dev, o, h)
                for h, group in zip(handles[:3], again):
                    for f, o in zip(forms, group):
                        f.case.launch(dev, o, h)
                other.launch(dev, oo, handles[0])
            finally:
                torch.cuda.synchronize()
            for k, group in enumerate(outs + again):
                for f, o in zip(forms, group):
                    _check(o, f.want, ("stream", k, f.name))
            _check(oo, owant, "stream 1, another palette")
            assert (owant["rgba"] != forms[0].want["rgba"]).mean() > 0.1
    finally:
        torch.cuda.synchronize()
        for h in made:                              # the ctx is closed
            assert hip.hipStreamDestroy(h) == 0
