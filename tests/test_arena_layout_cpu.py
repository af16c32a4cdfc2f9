"""The layout of a context's device arena (csrc/arena_layout.h), checked on the host: lay_out_arena is pure integer arithmetic, so a
host-only compile of a small program runs the very function gg_create runs, with a placer that records every region."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "groundgrid_amd")  # (the sweep's two sizes come from the built library's own host functions)


def test_arena_regions_are_aligned_disjoint_and_large_enough():
    src = os.path.join(ROOT, "tests", "cpp", "test_arena_layout.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "t")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "groundgrid_amd", "csrc"), src, "-o", exe, "-L", LIBDIR, "-lgroundgrid_hip", "-Wl,-rpath," + LIBDIR])
        out = subprocess.check_output([exe], text=True)
    assert out.strip() == "ok", out
