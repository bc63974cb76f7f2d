"""GPU tests of the compact form of the density replay (csrc/mbk_density.h, MBK_DENSITY_COMPACT=1: the qualifying samples
listed by count band with a counting and a scatter pass, then replayed 64 list entries to a wave), which does not ship and which
no other test builds.  A process keeps one library, so the second build (build.build_variant) runs every case of
tests/density_cases.py and the two band-loop views in ONE child process (tests/density_child.py), under a time limit; the tests
here compare what it wrote with the model (tests/density_model.py), exactly.  If the child ends by a signal, with a HIP error or
at its time limit, every test of the module fails with its output and nothing more is started on the GPU.

Time limit: the child's first clean run on an MI355X took CHILD_SECONDS_MEASURED s from start to exit (profiles/density/README.md);
the limit is about three times that."""
import os
import subprocess
import sys

import numpy as np
import pytest

import density_cases as DC

from distributedmandelbrot_amd import _lib as L
from distributedmandelbrot_amd import build as B

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_SECONDS_MEASURED = 4.8
CHILD_TIMEOUT = 15


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """What the child wrote: {key: array}; or why there is nothing, as a failure of every test that asks."""
    state = {}
    so = B.variant_path("density_compact")
    try:
        if B.needs_build(so):
            so = B.build_variant("density_compact", B.VARIANTS["density_compact"])   # raises without hipcc: no skip, no plain build
        out = str(tmp_path_factory.mktemp("density_compact") / "results.npz")
        cmd = [sys.executable, os.path.join(HERE, "density_child.py"), "--lib", so, "--out", out]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            state["error"] = f"the child did not end within {CHILD_TIMEOUT} s\nstdout: {e.stdout!r}\nstderr: {e.stderr!r}"
        else:
            if p.returncode != 0:
                how = f"signal {-p.returncode}" if p.returncode < 0 else f"exit status {p.returncode}"
                state["error"] = f"the child ended with {how}\nstdout:\n{p.stdout[-4000:]}\nstderr:\n{p.stderr[-4000:]}"
            else:
                with np.load(out) as z:
                    state["results"] = {k: z[k] for k in z.files}
                print(p.stdout)
    except Exception as e:   # the library could not be built
        state["error"] = f"no compact build: {e!r}"
    return state


def _results(child):
    if "error" in child:
        pytest.fail(child["error"], pytrace=False)
    return child["results"]


def _case(results, prefix):
    return {k[len(prefix) + 2:]: v for k, v in results.items() if k.startswith(prefix + "__")}


def test_the_child_ran_the_compact_form(child):
    """Without this a wrong path would compare the plain build with itself."""
    assert int(_results(child)["build_info"]) == 1
    assert L.load().mbk_density_build_info() == 0   # ... and this process holds the library that ships


@pytest.mark.parametrize("name", [c.name for c in DC.CASES])
def test_case_equals_the_model(child, name):
    got = _case(_results(child), name)
    assert got, name
    DC.check_case(DC.BY_NAME[name], got)


@pytest.mark.parametrize("which", [0, 1], ids=["rows", "cols"])
def test_band_loop_of_the_compact_build(child, oracle, which):
    """density_run with 8 bytes of scratch per sample: a view of two row bands (8192 x 4100: 4095 and 5 rows) and a row of
    33 556 000 samples, cut into two column tiles, against the host twin, the C oracle's statistics and the same view as two
    one-band window launches."""
    results = _results(child)
    name, view, windows = DC.band_views(8, L.MBK_RENDER_BAND_BYTES)[which]
    limit = (L.MBK_RENDER_BAND_BYTES - 1024) // 8
    if name == "rows":
        assert -(-view.height // (limit // view.width)) == 2
    else:
        assert view.width > limit and -(-view.width // limit) == 2
    got = _case(results, "band_" + name)
    print(f"compact band view {name}: {float(got['seconds']):.2f} s in the child, kernel_ms {float(got['kernel_ms']):.2f}")
    DC.check_band_view(oracle, view, got)
