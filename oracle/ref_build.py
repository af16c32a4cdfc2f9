"""Recipe for the reference build (TEST INFRASTRUCTURE): compiles oracle/ref_driver.cpp -- one translation unit that includes the
reference's own src/GroundSegmentation.cpp by path -- against the functional stand-ins of oracle/ref_shim/ into

    oracle/_ref/gg_ref_run            Eigen 3.3 order of the block sums, KDL rotation (the default conventions)
    oracle/_ref/gg_ref_run_eigen34    the Eigen 3.4 + SSE order (-DGG_REF_SHIM_EIGEN34)

The flags are those of oracle/Makefile transposed to C++17: -O2, SSE2 scalar math, no FMA contraction, no fast-math, no -march.
Nothing of the reference is copied: its files are read where they lie (GG_REFERENCE_DIR, default /root/reference), and
oracle/_ref/ stays out of git.  What this pins and what it does not: DESIGN.md §2.
"""
from __future__ import annotations

import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(_HERE, "_ref")
BINARIES = {"gg_ref_run": [], "gg_ref_run_eigen34": ["-DGG_REF_SHIM_EIGEN34"]}
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-variable", "-Wno-unused-parameter",
            "-Wno-unused-but-set-variable"]


def reference_dir() -> str:
    return os.environ.get("GG_REFERENCE_DIR", "/root/reference")


def reference_source() -> str:
    return os.path.join(reference_dir(), "src", "GroundSegmentation.cpp")


def have_reference() -> bool:
    return os.path.isfile(reference_source()) and os.path.isfile(os.path.join(reference_dir(), "include", "groundgrid", "GroundSegmentation.h"))


def binary(name: str = "gg_ref_run") -> str:
    return os.path.join(OUT_DIR, name)


def have_binaries() -> bool:
    return all(os.path.isfile(binary(n)) and os.access(binary(n), os.X_OK) for n in BINARIES)


def _inputs():
    files = [os.path.join(_HERE, "ref_driver.cpp"), os.path.abspath(__file__)]
    for d, _, names in os.walk(os.path.join(_HERE, "ref_shim")):
        files += [os.path.join(d, n) for n in names]
    if have_reference():
        files += [reference_source(), os.path.join(reference_dir(), "include", "groundgrid", "GroundSegmentation.h"),
                  os.path.join(reference_dir(), "include", "velodyne_pointcloud", "point_types.h")]
    return files


def build(force: bool = False) -> dict:
    """Compile the reference binaries; returns {name: path}.  Raises if the reference is not on this machine."""
    if not have_reference():
        raise FileNotFoundError(f"no reference under {reference_dir()} (GG_REFERENCE_DIR)")
    os.makedirs(OUT_DIR, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _inputs())
    cxx = os.environ.get("CXX", "g++")
    for name, defs in BINARIES.items():
        out = binary(name)
        if not force and os.path.isfile(out) and os.path.getmtime(out) >= newest:
            continue
        cmd = [cxx, *CXXFLAGS, *defs, f'-DGG_REFERENCE_SEGMENTATION_CPP="{reference_source()}"',
               "-I" + os.path.join(_HERE, "ref_shim"), "-I" + os.path.join(reference_dir(), "include"),
               os.path.join(_HERE, "ref_driver.cpp"), "-o", out + ".tmp", "-lm", "-lpthread"]
        subprocess.check_call(cmd)
        os.replace(out + ".tmp", out)
    return {n: binary(n) for n in BINARIES}


def ensure() -> bool:
    """True if the binaries are there (built now where the reference exists), False where neither they nor the reference exist."""
    if have_reference():
        build()
        return True
    return have_binaries()


if __name__ == "__main__":
    print(build(force=True))
