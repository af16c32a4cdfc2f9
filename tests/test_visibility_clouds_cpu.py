"""gg_visibility_clouds without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirror has the
layout the C compiler gives the struct, the ABI version and the neighbouring structs are what they were, a null context is refused before
the device is touched, and the Python entry point refuses bad arguments before any library call.  And the expectation of the GPU tests
(tests/visibility_ref.py) is held without the code under test: its closed form against exact rational arithmetic with halves rounded away
from zero, the shape of its paths, and its mirror symmetry."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, build  # noqa: E402
from tests import visibility_ref  # noqa: E402

FIELDS = ["n", "first_slot", "slots", "point_format", "d_points", "cloud_stride", "n_points", "transforms", "d_labels", "d_label_masks",
          "min_points", "min_height", "max_height", "origins", "max_cells", "order", "d_state", "plane_stride", "d_counts"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def compile_and_run(prog):
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        libdir = os.path.dirname(_lib.LIB_PATH)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t"),
                               "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
        return subprocess.run([os.path.join(d, "t")], stdout=subprocess.PIPE, check=True).stdout.decode()


# ---------------------------------------------------------------- the ABI

def test_symbol_is_exported_and_bound(lib):
    assert "gg_visibility_clouds" in _lib.SYMBOLS
    assert hasattr(lib, "gg_visibility_clouds")
    assert len(lib.gg_visibility_clouds.argtypes) == 3


def test_field_list_and_the_ten_leading_members():
    assert [f[0] for f in _lib.GGCloudVisibility._fields_] == FIELDS
    assert _lib.GGCloudVisibility._fields_[:10] == _lib.GGCloudRaster._fields_[:10]  # names and types
    assert (_lib.GG_CELL_FREE, _lib.GG_CELL_UNKNOWN, _lib.GG_CELL_OCCUPIED) == (-1, 0, 1) == (visibility_ref.FREE, visibility_ref.UNKNOWN, visibility_ref.OCCUPIED)


def test_struct_layout_equals_the_ctypes_mirror(lib):
    lines = ['printf("%zu\\n", sizeof(gg_cloud_visibility));']
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_visibility, {k}));' for k in FIELDS]
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_raster, {k}));' for k in FIELDS[:10]]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    got = [int(v) for v in out.split()]
    want = [C.sizeof(_lib.GGCloudVisibility)] + [getattr(_lib.GGCloudVisibility, k).offset for k in FIELDS]
    assert got[: len(want)] == want
    assert got[1:11] == got[len(want):]  # the ten leading members lie where gg_cloud_raster has them


def test_feature_macro_and_the_constants(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_VISIBILITY_CLOUDS) || GG_HAS_VISIBILITY_CLOUDS != 1
    #error "GG_HAS_VISIBILITY_CLOUDS"
    #endif
    int main(void) { printf("%d %d %d %d\n", GG_HAS_VISIBILITY_CLOUDS, GG_CELL_FREE, GG_CELL_UNKNOWN, GG_CELL_OCCUPIED); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, -1, 0, 1]


def test_abi_version_and_the_other_structs_are_unchanged(lib):
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { printf("%d %zu %zu %zu %zu %zu\n", GG_ABI_VERSION, sizeof(gg_batch), sizeof(gg_cloud_raster), sizeof(gg_cloud_split), sizeof(gg_cloud_clusters),
                            sizeof(gg_cloud_clearance)); return 0; }
    ''')
    version, batch, raster, split, clusters, clearance = (int(v) for v in out.split())
    assert version == 6
    assert batch == C.sizeof(_lib.GGBatch) == 120
    assert raster == C.sizeof(_lib.GGCloudRaster)
    assert split == C.sizeof(_lib.GGCloudSplit)
    assert clusters == C.sizeof(_lib.GGCloudClusters)
    assert clearance == C.sizeof(_lib.GGCloudClearance)


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <math.h>
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int step(gg_context *ctx, const gg_point16 *d_points, const uint8_t *d_labels, int32_t *d_state, int32_t *d_counts, void *stream) {
        const int32_t slots[2] = {3, 1}, n_points[2] = {1000, 64};
        const float origins[2][3] = {{0.f, 0.f, 1.7f}, {2.5f, -1.f, 1.7f}};
        gg_cloud_visibility x = {0};
        x.n = 2;
        x.slots = slots;
        x.point_format = GG_POINT16;
        x.d_points = d_points;
        x.cloud_stride = 1024;
        x.n_points = n_points;
        x.d_labels = d_labels;
        x.min_points = 2;
        x.min_height = 0.3f;
        x.max_height = INFINITY;
        x.origins = &origins[0][0];
        x.max_cells = 30;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_state = d_state;
        x.plane_stride = 364 * 364;
        x.d_counts = d_counts;
        return gg_visibility_clouds(ctx, &x, stream);
    }
    int main(void) { return step(NULL, NULL, NULL, NULL, NULL, GG_STREAM_DEFAULT) == GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGCloudVisibility()
    x.n = 1
    assert lib.gg_visibility_clouds(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_visibility_clouds(None, None, None) == -1
    x.n = 0
    assert lib.gg_visibility_clouds(None, C.byref(x), None) == -1


# ---------------------------------------------------------------- the Python entry point

def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.visibility_clouds).parameters
    assert list(params)[:4] == ["self", "points", "n_points", "origins"]
    defaults = {"labels": None, "masks": None, "transforms": None, "slots": None, "first_slot": 0, "min_points": 1, "min_height": -math.inf,
                "max_height": math.inf, "max_cells": 0, "order": "row", "counts": True, "out": None, "on_torch_stream": True}
    assert list(params)[4:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert [f for f in api.VisibilityOutputs.__dataclass_fields__] == ["state", "counts"]


class NoLibrary:
    """in place of the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


def test_python_entry_point_refuses_bad_arguments_before_any_library_call(lib):
    import torch

    seg = api.GroundSegmentation()
    seg._L, seg.rows, seg.cols, seg.device = NoLibrary(), 79, 79, 0
    points = torch.zeros((2, 64, 16), dtype=torch.uint8)
    labels = torch.zeros((2, 64), dtype=torch.uint8)
    good = np.zeros((2, 3), np.float32)
    for kw in (dict(order="fortran"), dict(max_cells=-1), dict(max_cells=1.5), dict(min_points=0), dict(min_height=math.nan), dict(max_height=math.nan)):
        with pytest.raises(ValueError):
            seg.visibility_clouds(points, [64, 64], good, labels=labels, **kw)
    for origins in (None, np.zeros((2, 2), np.float32), np.zeros((3, 3), np.float32), np.zeros(6, np.float32), [[0.0, 0.0, 0.0]], "here",
                    [[0.0, 0.0, 0.0], [1.0, 2.0]], np.zeros((2, 3, 1), np.float32)):
        with pytest.raises(ValueError):
            seg.visibility_clouds(points, [64, 64], origins, labels=labels)


# ---------------------------------------------------------------- the reference, without the code under test

ORIGINS = [(0, 0), (20, 20), (40, 3), (17, 29)]
SIZE = 41


def rounded_half_away(q):
    """a Fraction rounded to the nearest integer, halves away from zero"""
    s = -1 if q < 0 else 1
    return s * int(math.floor(abs(q) + Fraction(1, 2)))


def path_by_fractions(r0, c0, r1, c1):
    dr, dc = r1 - r0, c1 - c0
    n = max(abs(dr), abs(dc))
    return [(r0 + rounded_half_away(Fraction(k * dr, n)), c0 + rounded_half_away(Fraction(k * dc, n))) for k in range(n)]


def path_of(r0, c0, r1, c1, max_cells=0):
    rr, cc = visibility_ref.ray_cells(r0, c0, r1, c1, max_cells)
    return list(zip(rr.tolist(), cc.tolist()))


@pytest.mark.parametrize("origin", ORIGINS)
def test_closed_form_equals_exact_rounding(origin):
    r0, c0 = origin
    halves = 0
    for r1 in range(SIZE):
        for c1 in range(SIZE):
            path = path_of(r0, c0, r1, c1)
            assert path == path_by_fractions(r0, c0, r1, c1), (origin, r1, c1)
            n, m = max(abs(r1 - r0), abs(c1 - c0)), min(abs(r1 - r0), abs(c1 - c0))
            halves += sum(1 for k in range(n) if (2 * k * m) % n == 0 and ((2 * k * m) // n) % 2 == 1)  # k m / n lies on an exact half
    assert halves > 100  # (the tie rule decided somewhere)


@pytest.mark.parametrize("origin", ORIGINS)
def test_paths_are_connected_and_stop_short_of_the_end_cell(origin):
    r0, c0 = origin
    for r1 in range(SIZE):
        for c1 in range(SIZE):
            path = path_of(r0, c0, r1, c1)
            n = max(abs(r1 - r0), abs(c1 - c0))
            assert len(path) == n
            if n == 0:
                continue
            assert path[0] == (r0, c0) and (r1, c1) not in path
            chain = path + [(r1, c1)]
            assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(chain, chain[1:])), (origin, r1, c1)
            for R in (1, 7):
                assert path_of(r0, c0, r1, c1, R) == path[:R]


def test_paths_mirror_under_the_eight_reflections():
    reflections = [lambda a, b: (a, b), lambda a, b: (-a, b), lambda a, b: (a, -b), lambda a, b: (-a, -b),
                   lambda a, b: (b, a), lambda a, b: (-b, a), lambda a, b: (b, -a), lambda a, b: (-b, -a)]
    for dr in range(0, 41):
        for dc in range(0, dr + 1):
            base = path_of(0, 0, dr, dc)
            for f in reflections:
                assert path_of(0, 0, *f(dr, dc)) == [f(a, b) for a, b in base], (dr, dc)


def test_a_sub_ray_is_in_general_no_prefix():
    """why the end cells have to be fixed before anything is traced: the ray to a crossed cell leaves the ray that crossed it"""
    with_other_sub_ray = 0
    for r1 in range(SIZE):
        for c1 in range(SIZE):
            path = path_of(20, 20, r1, c1)
            with_other_sub_ray += any(path_of(20, 20, *cell) != path[:k] for k, cell in enumerate(path))
    assert with_other_sub_ray == 1368


# ---------------------------------------------------------------- fixed facts of the expectation

def test_occupied_beats_free_and_counts_add_up():
    occupied, hit = np.zeros((9, 9), bool), np.zeros((9, 9), bool)
    occupied[4, 6] = hit[4, 6] = hit[4, 8] = True
    state, counts = visibility_ref.expected_visibility(occupied, hit, (4, 2), 0, "row")
    assert state[4].tolist() == [0, 0, -1, -1, -1, -1, 1, -1, -1]  # the ray to (4, 8) passes the occupied cell, which stays occupied
    assert counts.tolist() == [6, 74, 1] and int(np.abs(state).sum()) == 7
    col, counts_col = visibility_ref.expected_visibility(occupied, hit, (4, 2), 0, "col")
    assert np.array_equal(col, state.T) and np.array_equal(counts, counts_col)
    near, _ = visibility_ref.expected_visibility(occupied, hit, (4, 2), 2, "row")
    assert near[4].tolist() == [0, 0, -1, -1, 0, 0, 1, 0, -1]  # two cells of every ray, and the hits themselves


def test_a_sensor_in_no_cell_frees_exactly_the_hits_that_are_not_occupied():
    for name, scene in visibility_ref.scenes().items():
        occupied, hit, origin = visibility_ref.scene_truth(scene)
        state, counts = visibility_ref.expected_visibility(occupied, hit, None, 0, "row")
        assert np.array_equal(state == -1, hit & ~occupied) and np.array_equal(state == 1, occupied), name
        assert int(counts.sum()) == 79 * 79
        if scene["sensor"] in (visibility_ref.OUTSIDE, visibility_ref.NOT_FINITE):
            assert origin is None and hit.any()
