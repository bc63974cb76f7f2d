"""GPU tests of density views (include/mbk.h, "Density views"): the device tables against the numpy restatement of the
contract in tests/density_model.py -- and against the host twin where that is cheap --, exactly."""
import numpy as np
import pytest

import density_cases as DC
import density_model as M
from density_cases import BIG, DISC, MRD, NARROW, VIEW, WIDE

from distributedmandelbrot_amd import DensityTarget, MandelbrotDevice, MbkError, Palette, View
from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd.device import density_host
from distributedmandelbrot_amd.sharding import accumulate_view_density

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def reference():
    """The model's tables, computed once and shared (read-only)."""
    out = {}
    for name, target in (("wide", WIDE), ("narrow", NARROW)):
        out[name] = M.accumulate(VIEW, target, MRD)
    out["big"] = M.accumulate(BIG, WIDE, MRD)
    for v in out.values():
        v[0].setflags(write=False)
    return out


def _device_table(gpu, view, target, mrd, launches, guard=64, **kw):
    """The table after `launches` (a list of windows, None = the whole view) into one cleared device table with `guard`
    sentinel words on either side; the sentinels are checked."""
    table, intact, buf = DC.device_table(gpu, view, target, mrd, launches, guard=guard, **kw)
    assert intact, "a word outside the table was written"
    return table, buf


def test_this_is_the_plain_form(gpu):
    """The library that ships replays one lane per sample (tests/test_gpu_density_compact.py runs the other form)."""
    assert gpu._lib.mbk_density_build_info() == 0


@pytest.mark.parametrize("name", [c.name for c in DC.CASES])
def test_case_equals_the_model(gpu, name):
    """Every case of tests/density_cases.py -- the shapes chosen for the list kernels of the compact form, the wrap at 2^32 and
    the table's edges among them -- on the plain form."""
    case = DC.BY_NAME[name]
    DC.check_case(case, DC.run_case(gpu, case))


def test_table_edges_against_their_integer_restatement(gpu):
    """View (-1, -1, 2, 2, 9, 9) into 8 x 8 cells of the same square: z_0 = (i / 4 - 1, j / 4 - 1) is the lower left corner of
    cell (i, j), column 8 and row 8 lie exactly on the right and the top edge and are dropped, and row 0 holds the samples with
    c_i = -1.  At mrd 2 with min_count = max_count = 1 only z_0 of the n = 1 samples is deposited.  The same with the target moved
    by half a cell, where z_0 is the centre of cell (i, j)."""
    n = DC.view_counts(DC.NINE, 2)
    want = (n[:8, :8] == 1).astype(np.uint32)
    assert want[0].any() and (n[:, 8] == 1).all() and (n[8] == 1).any()
    for name in ("edge", "edge_half"):
        case = DC.BY_NAME[name]
        got, _ = _device_table(gpu, case.view, case.target, 2, [None], min_count=1, max_count=1)
        assert np.array_equal(got, want), name
        table, _, ds = gpu.compute_view_density(case.view, case.target, 2, min_count=1, max_count=1)
        assert np.array_equal(table, want) and (ds.deposits, ds.dropped) == (int(want.sum()), int((n == 1).sum()) - int(want.sum()))


def test_a_launch_adds_modulo_2_to_the_32(gpu):
    small = DC.BY_NAME["wrap_all"]
    model = DC.expected(DC.BY_NAME["partial"])[0].astype(np.int64)
    got, _ = _device_table(gpu, small.view, small.target, small.mrd, [None], init=DC.initial(small))
    assert model.any() and np.array_equal(got.astype(np.int64), (model - 1) % 2 ** 32)
    word = DC.BY_NAME["wrap_word"]
    want = DC.expected(word)[0]
    got, buf = _device_table(gpu, word.view, word.target, word.mrd, [None], init=DC.initial(word))
    assert np.array_equal(got, want) and int(want.ravel()[DC.WRAP_WORD]) == int(DC.expected(DC.BY_NAME["wide"])[0].max()) - 16
    assert gpu.density_max(buf.data_ptr() + 4 * 64, got.size) == (int(want.max()), int(want.astype(np.uint64).sum()))
    assert int(want.max()) < 2 ** 31   # the word that passed 2^32 is small again


@pytest.mark.parametrize("which", [0, 1], ids=["rows", "cols"])
def test_band_loop_of_density_run(gpu, oracle, which):
    """density_run past one band of the count scratch (MBK_RENDER_BAND_BYTES - 1024 bytes, 4 per sample): 8192 x 8200 samples are
    two row bands of 8191 and 9 rows, a row of 67 110 000 samples two column tiles.  At mrd 8 into 512 x 512 cells that hold the
    disc of radius 2: against the host twin's table, the C oracle's statistics, and the same view as two one-band windows."""
    name, view, windows = DC.band_views(4, L.MBK_RENDER_BAND_BYTES)[which]
    limit = (L.MBK_RENDER_BAND_BYTES - 1024) // 4
    if name == "rows":
        assert -(-view.height // (limit // view.width)) == 2
    else:
        assert view.width > limit and -(-view.width // limit) == 2
    got = DC.run_band_view(gpu, view, windows)
    print(f"plain band view {name}: kernel_ms {got['kernel_ms']:.2f}")
    DC.check_band_view(oracle, view, got)


@pytest.mark.parametrize("kernel", ["default", "asm", "group", "scan"])
@pytest.mark.parametrize("name,target", [("wide", WIDE), ("narrow", NARROW)])
def test_tables_equal_the_model_with_every_kernel(gpu, reference, kernel, name, target):
    want, dep, drop, n = reference[name]
    got, st, ds = gpu.compute_view_density(VIEW, target, MRD, kernel=kernel)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert (ds.deposits, ds.dropped) == (dep, drop) and dep + drop == int(n.sum())
    assert st.never_pixels == int((n == 0).sum())
    assert st.pixel_iterations == int(n.sum()) + (MRD - 1) * st.never_pixels
    if kernel == "default":
        host, hs = density_host(VIEW, target, MRD)
        assert np.array_equal(got, host) and (hs.deposits, hs.dropped) == (dep, drop)


def test_partial_blocks(gpu):
    small = View(-2.0, -1.25, 3.0, 2.5, 13, 9)
    want, dep, drop, _ = M.accumulate(small, WIDE, MRD)
    got, _, ds = gpu.compute_view_density(small, WIDE, MRD)
    assert np.array_equal(got, want) and (ds.deposits, ds.dropped) == (dep, drop)


def test_windows_and_launches_add_up(gpu, reference):
    want = reference["big"][0]
    whole, _ = _device_table(gpu, BIG, WIDE, MRD, [None])
    bands, _ = _device_table(gpu, BIG, WIDE, MRD, [(0, 0, 100, 23), (0, 23, 100, 24), (0, 47, 100, 23)])
    cols, _ = _device_table(gpu, BIG, WIDE, MRD, [(0, 0, 9, 70), (9, 0, 41, 70), (50, 0, 49, 70), (99, 0, 1, 70)])
    assert np.array_equal(whole, want) and np.array_equal(bands, want) and np.array_equal(cols, want)
    window = (17, 11, 30, 21)
    once, _ = _device_table(gpu, BIG, WIDE, MRD, [window])
    twice, _ = _device_table(gpu, BIG, WIDE, MRD, [window, window])
    assert np.array_equal(once, M.accumulate(BIG, WIDE, MRD, window=window)[0]) and np.array_equal(twice, 2 * once)


def test_contention_and_bounds(gpu, reference):
    inner = View(-1.9, -1.2, 2.4, 2.4, 48, 40)
    n = M.accumulate(inner, DISC, MRD)[3]
    one, _, ds = gpu.compute_view_density(inner, DensityTarget(-2.5, -2.5, 5.0, 5.0, 1, 1), MRD)
    assert one.shape == (1, 1) and int(one[0, 0]) == int(n.sum()) == ds.deposits and ds.dropped == 0
    t22 = DensityTarget(-2.5, -2.5, 5.0, 5.0, 2, 2)
    four, _ = _device_table(gpu, inner, t22, MRD, [None])
    assert np.array_equal(four, M.accumulate(inner, t22, MRD, n=n)[0]) and int(four.sum()) == int(n.sum())
    # most points fall outside a 17 x 5 table: the sentinels around it stay (checked by _device_table)
    t175 = DensityTarget(-0.3, 0.55, 0.31, 0.2, 17, 5)
    want, dep, drop, _ = M.accumulate(VIEW, t175, MRD, n=reference["wide"][3])
    got, _ = _device_table(gpu, VIEW, t175, MRD, [None], guard=256)
    assert np.array_equal(got, want) and drop > 10 * dep > 0


@pytest.mark.parametrize("mrd", [0, 1, 2, 3, 258])
def test_the_ends_of_the_loop(gpu, mrd):
    view = View(-2.0, -1.25, 3.0, 2.5, 40, 24)
    want, dep, drop, n = M.accumulate(view, WIDE, mrd)
    got, st, ds = gpu.compute_view_density(view, WIDE, mrd)
    assert np.array_equal(got, want) and (ds.deposits, ds.dropped) == (dep, drop)
    assert st.never_pixels == int((n == 0).sum())
    if mrd < 2:
        assert not got.any()
    else:
        assert dep > 0
        top, _, _ = gpu.compute_view_density(view, WIDE, mrd, min_count=mrd - 1, max_count=mrd - 1)
        assert np.array_equal(top, M.accumulate(view, WIDE, mrd, mrd - 1, mrd - 1, n=n)[0])


def test_a_row_with_a_subnormal_imaginary_part(gpu):
    """Where c_i is subnormal the fused doubling fma(2, zr zi, c_i) and the literal fl(fl(2 zr) zi) + c_i differ; the counts come
    from the literal kernels there and the replay is literal everywhere."""
    view = View(-2.0, -3e-310, 2.5, 6e-310, 40, 3)
    ys = M.axes(view)[1]
    assert ((ys != 0.0) & (np.abs(ys) < 2.0 ** -1022)).any()
    flat = DensityTarget(-2.0, -1e-300, 2.5, 2e-300, 64, 8)
    for target in (flat, WIDE):
        want, dep, drop, _ = M.accumulate(view, target, 120)
        got, _, ds = gpu.compute_view_density(view, target, 120)
        assert np.array_equal(got, want) and (ds.deposits, ds.dropped) == (dep, drop) and dep > 0


def test_launch_on_a_stream_equals_compute_and_density_max(gpu, reference):
    torch = _torch()
    want = reference["wide"][0]
    stream = torch.cuda.Stream()
    buf = torch.zeros(WIDE.width * WIDE.height, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gpu.launch_view_density(VIEW, WIDE, MRD, d_density=buf.data_ptr(), stream=stream.cuda_stream)
        mx, total = gpu.density_max(buf.data_ptr(), buf.numel(), stream=stream.cuda_stream)
    stream.synchronize()
    got = buf.cpu().numpy().view(np.uint32).reshape(want.shape)
    assert np.array_equal(got, want) and np.array_equal(got, gpu.compute_view_density(VIEW, WIDE, MRD)[0])
    assert (mx, total) == (int(want.max()), int(want.sum()))
    assert gpu.density_max(buf.data_ptr(), 0) == (0, 0)
    # values near 2^32 and a length that is no multiple of anything
    rs = np.random.RandomState(2)
    big = rs.randint(0, 2 ** 32, 100003, dtype=np.uint64).astype(np.uint32)
    d = torch.from_numpy(big.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    assert gpu.density_max(d.data_ptr(), big.size) == (int(big.max()), int(big.astype(np.uint64).sum()))


@pytest.mark.parametrize("mode", ["sqrt", "linear"])
@pytest.mark.parametrize("factor", [1, 4])
def test_render_density_equals_the_model(gpu, reference, mode, factor):
    torch = _torch()
    table = np.array(reference["wide"][0], np.uint32)
    table[0, 0], table[1, 1] = 2 ** 32 - 1, 0
    rs = np.random.RandomState(9)
    entries = rs.randint(0, 256, (300, 4)).astype(np.uint8)
    pal = Palette(entries).for_density(int(np.sort(table.ravel())[-2]), mode)
    want = M.render(entries, pal.scale, pal.offset, mode, factor, table)
    got, _ = gpu.render_density(table, palette=pal, mode=mode, factor=factor)
    assert got.shape == want.shape and np.array_equal(got, want)
    d_table = torch.from_numpy(table.view(np.int32)).to("cuda:0")
    img = torch.full((64 + want.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.launch_render_density(d_table.data_ptr(), WIDE.width, WIDE.height, palette=pal, d_rgba=img.data_ptr() + 64, mode=mode, factor=factor)
    torch.cuda.synchronize()
    back = img.cpu().numpy()
    assert (back[:64] == 0xA5).all() and (back[64 + want.size:] == 0xA5).all()
    assert np.array_equal(back[64:64 + want.size].reshape(want.shape), want)


def test_two_contexts_on_one_gpu_sum_to_the_single_table(gpu, reference):
    with MandelbrotDevice(0) as other:
        got, per_dev = accumulate_view_density([gpu, other], BIG, WIDE, MRD, band_rows=9)
    want, dep, drop, _ = reference["big"]
    assert np.array_equal(got, want)
    assert sum(d["deposits"] for d in per_dev) == dep and sum(d["dropped"] for d in per_dev) == drop
    assert sum(d["bands"] for d in per_dev) == 8


def test_refusals_leave_the_context_usable(gpu, oracle):
    import ctypes as C
    torch = _torch()
    buf = torch.full((WIDE.width * WIDE.height,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    cv, ct = gpu._cview(VIEW, None), WIDE.ctarget()
    lib = gpu._lib

    def launch(flags, mrd=MRD, lo=1, hi=0, ptr=None, target=ct):
        return lib.mbk_view_density_launch(gpu._h, C.byref(cv), C.byref(target), mrd, lo, hi, flags, buf.data_ptr() if ptr is None else ptr, None)

    bad = L.MBK_ERR_INVALID
    for flags in (L.MBK_DEEP_BLA, L.MBK_PRECISION_F32, L.MBK_LAZY_UNIFORM, L.MBK_KERNEL_SIMPLE, L.MBK_KERNEL_REFILL, 0x600, L.MBK_WANT_COUNTS):
        assert launch(flags) == bad, hex(flags)
        host = np.full((WIDE.height, WIDE.width), 7, np.uint32)
        assert lib.mbk_view_density_compute(gpu._h, C.byref(cv), C.byref(ct), MRD, 1, 0, flags, host.ctypes.data, None, None) == bad
        assert (host == 7).all()
    assert launch(0, lo=0) == bad and launch(0, lo=9, hi=8) == bad and launch(0, hi=MRD) == bad and launch(0, mrd=2 ** 31) == bad
    assert launch(0, ptr=buf.data_ptr() + 2) == bad
    assert launch(0, target=L.mbk_density_target(-2.0, -1.5, 0.0, 3.0, 48, 40)) == bad
    assert lib.mbk_view_density_launch(gpu._h, C.byref(cv), C.byref(ct), MRD, 1, 0, 0, None, None) == bad
    mx, total = C.c_uint32(0), C.c_uint64(0)
    assert lib.mbk_density_max(gpu._h, buf.data_ptr() + 1, 4, C.byref(mx), C.byref(total), None) == bad
    with pytest.raises(MbkError):
        gpu.render_density(np.zeros((8, 8), np.uint32), palette=Palette(np.zeros((4, 4), np.uint8)), factor=3)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 7).all()
    # the ctx still computes an ordinary view
    counts, _, st = gpu.compute_view(VIEW, MRD, want_bytes=False)
    oc, _, total = oracle.view(VIEW.start_r, VIEW.start_i, VIEW.range_r, VIEW.range_i, VIEW.width, VIEW.height, MRD)
    assert np.array_equal(counts, oc.reshape(counts.shape)) and st.pixel_iterations == total
