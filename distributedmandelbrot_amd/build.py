"""Build libmbk_hip.so (the HIP kernels + C ABI) in-tree with hipcc for gfx950.

    python -m distributedmandelbrot_amd.build [--force] [--save-temps]

The .so is git-ignored but travels to the GPU box with the gpurun snapshot.
-ffp-contract=off is MANDATORY: hipcc contracts a*b+c into v_fma_f64 by default, which would change
iteration counts (SURVEY.md probe P2).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libmbk_hip.so")
SOURCES = [os.path.join(CSRC, "mbk_api.hip")]
DEPS = (SOURCES + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")))
        + [os.path.join(os.path.dirname(HERE), "include", "mbk.h")])
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-fPIC", "-shared", "-Wall", "-Wno-unused-result"]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libmbk_hip.so")
    return exe


def needs_build(so: str = SO) -> bool:
    if not os.path.exists(so):
        return True
    t = os.path.getmtime(so)
    return any(os.path.getmtime(d) > t for d in DEPS if os.path.exists(d))


def build(force: bool = False, save_temps: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return SO
    cmd = [hipcc()] + FLAGS + SOURCES + ["-o", SO]
    cwd = HERE
    if save_temps:   # intermediate .s / .bc files go to the git-ignored build/ directory
        cwd = os.path.join(HERE, "build")
        os.makedirs(cwd, exist_ok=True)
        cmd += ["-save-temps=cwd", "-Rpass-analysis=kernel-resource-usage"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=cwd)
    return SO


# Second builds of the same sources under compile-time switches, for A/B runs and for the tests of a form that does not ship.
VARIANTS = {"density_compact": ["-DMBK_DENSITY_COMPACT=1"]}   # csrc/mbk_density.h: the compacted replay


def variant_path(name: str) -> str:
    return os.path.join(HERE, "build", f"libmbk_hip_{name}.so")


def build_variant(name: str, defines, force: bool = False, verbose: bool = False) -> str:
    """The same FLAGS and SOURCES plus `defines` (a list of -D... options) into the git-ignored build/libmbk_hip_<name>.so,
    rebuilt under the rule of build().  The shipped library is not touched."""
    so = variant_path(name)
    if not force and not needs_build(so):
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    cmd = [hipcc()] + FLAGS + list(defines) + SOURCES + ["-o", so]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=os.path.dirname(so))
    return so


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, save_temps="--save-temps" in sys.argv, verbose=True))
