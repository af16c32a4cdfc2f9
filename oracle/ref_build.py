"""Recipe for the reference build (TEST INFRASTRUCTURE): compiles oracle/ref_driver.cpp -- one translation unit that includes the
reference's own src/GroundSegmentation.cpp by path -- against the functional stand-ins of oracle/ref_shim/ into

    oracle/_ref/gg_ref_run            Eigen 3.3 order of the block sums, KDL rotation (the default conventions)
    oracle/_ref/gg_ref_run_eigen34    the Eigen 3.4 + SSE order (-DGG_REF_SHIM_EIGEN34)
    oracle/_ref/gg_ref_run_geomA      the default conventions with the two constants of the reference's GroundSegmentation.h:69-70
    oracle/_ref/gg_ref_run_geomB      at another pair of values (VARIANTS): they are compile-time constants, so one binary per pair

A variant is built from a SHADOW of that one header, written to oracle/_ref/<variant>/groundgrid/ with the two initialisers replaced
and put first on the include path; the reference's .cpp is still read where it lies, unmodified.

The flags are those of oracle/Makefile transposed to C++17: -O2, SSE2 scalar math, no FMA contraction, no fast-math, no -march.
Nothing of the reference is copied: its files are read where they lie (GG_REFERENCE_DIR, default /root/reference), and
oracle/_ref/ stays out of git.  What this pins and what it does not: DESIGN.md §2.
"""
from __future__ import annotations

import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(_HERE, "_ref")
BINARIES = {"gg_ref_run": [], "gg_ref_run_eigen34": ["-DGG_REF_SHIM_EIGEN34"]}
# variant -> (vertical_point_ang_dist, min_dist_squared) as floats: constant sets A and B of tests/geom_sets.py (which asserts the match)
VARIANTS = {"gg_ref_run_geomA": (0.00174532925, 446.0), "gg_ref_run_geomB": (0.00174532925 * 4, 264.0625)}
# the two members whose initialisers a shadow header replaces (everything between `=` and `;`)
_MEMBERS = ("verticalPointAngDist", "minDistSquared")
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
    return all(os.path.isfile(binary(n)) and os.access(binary(n), os.X_OK) for n in list(BINARIES) + list(VARIANTS))


def _float_literal(v) -> str:
    """the float nearest to v as a C++17 hexadecimal literal: exact, whatever the decimal digits"""
    import struct

    f = struct.unpack("<f", struct.pack("<f", float(v)))[0]
    return f.hex() + "f"


def reference_header() -> str:
    return os.path.join(reference_dir(), "include", "groundgrid", "GroundSegmentation.h")


def shadow_include_dir(variant: str) -> str:
    return os.path.join(OUT_DIR, variant.replace("gg_ref_run_", ""))


def write_shadow_header(variant: str) -> str:
    """oracle/_ref/<variant>/groundgrid/GroundSegmentation.h: the reference's header with the two initialisers replaced, nothing else.
    Raises unless exactly two lines changed, one per member.  Returns the include directory."""
    with open(reference_header()) as f:
        lines = f.read().split("\n")
    out, changed = [], []
    for line in lines:
        new = line
        for member, value in zip(_MEMBERS, VARIANTS[variant]):
            new, k = re.subn(r"(\b" + member + r"\s*=)[^;]*;", r"\g<1> " + _float_literal(value) + ";", new, count=1)
            if k and new != line:
                changed.append(member)
        out.append(new)
    if sorted(changed) != sorted(_MEMBERS):
        raise RuntimeError(f"{variant}: the substitution changed {changed}, expected exactly one line for each of {_MEMBERS}")
    inc = shadow_include_dir(variant)
    os.makedirs(os.path.join(inc, "groundgrid"), exist_ok=True)
    with open(os.path.join(inc, "groundgrid", "GroundSegmentation.h"), "w") as f:
        f.write("\n".join(out))
    return inc


def _inputs():
    files = [os.path.join(_HERE, "ref_driver.cpp"), os.path.abspath(__file__)]
    for d, _, names in os.walk(os.path.join(_HERE, "ref_shim")):
        files += [os.path.join(d, n) for n in names]
    if have_reference():
        files += [reference_source(), reference_header(),
                  os.path.join(reference_dir(), "include", "velodyne_pointcloud", "point_types.h")]
    return files


def build(force: bool = False) -> dict:
    """Compile the reference binaries; returns {name: path}.  Raises if the reference is not on this machine."""
    if not have_reference():
        raise FileNotFoundError(f"no reference under {reference_dir()} (GG_REFERENCE_DIR)")
    os.makedirs(OUT_DIR, exist_ok=True)
    newest = max(os.path.getmtime(f) for f in _inputs())
    cxx = os.environ.get("CXX", "g++")
    for name, defs in list(BINARIES.items()) + [(v, []) for v in VARIANTS]:
        out = binary(name)
        if not force and os.path.isfile(out) and os.path.getmtime(out) >= newest:
            continue
        shadow = ["-I" + write_shadow_header(name)] if name in VARIANTS else []   # first on the include path
        cmd = [cxx, *CXXFLAGS, *defs, f'-DGG_REFERENCE_SEGMENTATION_CPP="{reference_source()}"', *shadow,
               "-I" + os.path.join(_HERE, "ref_shim"), "-I" + os.path.join(reference_dir(), "include"),
               os.path.join(_HERE, "ref_driver.cpp"), "-o", out + ".tmp", "-lm", "-lpthread"]
        subprocess.check_call(cmd)
        os.replace(out + ".tmp", out)
    return {n: binary(n) for n in list(BINARIES) + list(VARIANTS)}


def ensure() -> bool:
    """True if the binaries are there (built now where the reference exists), False where neither they nor the reference exist."""
    if have_reference():
        build()
        return True
    return have_binaries()


if __name__ == "__main__":
    print(build(force=True))
