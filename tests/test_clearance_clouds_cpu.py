"""gg_clearance_clouds without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirror has the
layout the C compiler gives the struct, the ABI version and the neighbouring structs are what they were, a null context is refused before
the device is touched, and the Python entry points refuse bad arguments before any library call.  And the expectation of the GPU tests
(tests/clearance_ref.py) is held against scipy.ndimage.distance_transform_edt on every pattern those tests run, and its tie rule against an
independent loop per cell, without the code under test."""
import ctypes as C
import inspect
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, build  # noqa: E402
from tests import clearance_ref  # noqa: E402

FIELDS = ["n", "first_slot", "slots", "point_format", "d_points", "cloud_stride", "n_points", "transforms", "d_labels", "d_label_masks",
          "min_points", "min_height", "max_height", "d_seeds", "seed_stride", "max_cells", "order", "d_dist2", "plane_stride", "d_nearest",
          "d_distance", "d_n_occupied"]


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


def test_symbol_is_exported_and_bound(lib):
    assert "gg_clearance_clouds" in _lib.SYMBOLS
    assert hasattr(lib, "gg_clearance_clouds")
    assert len(lib.gg_clearance_clouds.argtypes) == 3


def test_field_list_and_the_ten_leading_members():
    assert [f[0] for f in _lib.GGCloudClearance._fields_] == FIELDS
    assert _lib.GGCloudClearance._fields_[:10] == _lib.GGCloudRaster._fields_[:10]  # names and types
    assert _lib.GG_CLEARANCE_NONE == 0x7FFFFFFF == clearance_ref.NONE


def test_struct_layout_equals_the_ctypes_mirror(lib):
    lines = ['printf("%zu\\n", sizeof(gg_cloud_clearance));']
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_clearance, {k}));' for k in FIELDS]
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_raster, {k}));' for k in FIELDS[:10]]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    got = [int(v) for v in out.split()]
    want = [C.sizeof(_lib.GGCloudClearance)] + [getattr(_lib.GGCloudClearance, k).offset for k in FIELDS]
    assert got[: len(want)] == want
    assert got[1:11] == got[len(want):]  # the ten leading members lie where gg_cloud_raster has them


def test_feature_macro_and_the_constant(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_CLEARANCE_CLOUDS) || GG_HAS_CLEARANCE_CLOUDS != 1
    #error "GG_HAS_CLEARANCE_CLOUDS"
    #endif
    int main(void) { printf("%d %d\n", GG_HAS_CLEARANCE_CLOUDS, GG_CLEARANCE_NONE); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, 0x7FFFFFFF]


def test_abi_version_and_the_other_structs_are_unchanged(lib):
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { printf("%d %zu %zu %zu %zu\n", GG_ABI_VERSION, sizeof(gg_batch), sizeof(gg_cloud_raster), sizeof(gg_cloud_split), sizeof(gg_cloud_clusters)); return 0; }
    ''')
    version, batch, raster, split, clusters = (int(v) for v in out.split())
    assert version == 6
    assert batch == C.sizeof(_lib.GGBatch) == 120
    assert raster == C.sizeof(_lib.GGCloudRaster)
    assert split == C.sizeof(_lib.GGCloudSplit)
    assert clusters == C.sizeof(_lib.GGCloudClusters)


def test_a_c_program_fills_the_struct_in_both_modes_and_links(lib):
    compile_and_run(r'''
    #include <math.h>
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int step(gg_context *ctx, const gg_point16 *d_points, const uint8_t *d_labels, const int32_t *d_seeds, int32_t *d_dist2, int32_t *d_nearest,
             float *d_distance, int32_t *d_counts, void *stream) {
        const int32_t slots[2] = {3, 1}, n_points[2] = {1000, 64};
        gg_cloud_clearance x = {0};
        x.n = 2;                       /* cloud mode */
        x.slots = slots;
        x.point_format = GG_POINT16;
        x.d_points = d_points;
        x.cloud_stride = 1024;
        x.n_points = n_points;
        x.d_labels = d_labels;
        x.min_points = 2;
        x.min_height = 0.3f;
        x.max_height = INFINITY;
        x.max_cells = 30;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_dist2 = d_dist2;
        x.plane_stride = 364 * 364;
        x.d_nearest = d_nearest;
        x.d_distance = d_distance;
        x.d_n_occupied = d_counts;
        int rc = gg_clearance_clouds(ctx, &x, stream);
        gg_cloud_clearance y = {0};
        y.n = 2;                       /* seed mode */
        y.d_seeds = d_seeds;
        y.seed_stride = 364 * 364 + 1;
        y.order = GG_PLANES_COLMAJOR;
        y.d_dist2 = d_dist2;
        y.plane_stride = 364 * 364;
        return rc + gg_clearance_clouds(ctx, &y, GG_STREAM_DEFAULT);
    }
    int main(void) { return step(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 2 * GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGCloudClearance()
    x.n = 1
    assert lib.gg_clearance_clouds(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_clearance_clouds(None, None, None) == -1
    x.n = 0
    assert lib.gg_clearance_clouds(None, C.byref(x), None) == -1


def test_python_entry_points_exist():
    params = inspect.signature(api.GroundSegmentation.clearance_clouds).parameters
    assert list(params)[:3] == ["self", "points", "n_points"]
    defaults = {"labels": None, "masks": None, "transforms": None, "slots": None, "first_slot": 0, "min_points": 1, "min_height": -math.inf,
                "max_height": math.inf, "max_cells": 0, "order": "row", "nearest": True, "distance": True, "out": None, "on_torch_stream": True}
    assert list(params)[3:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    params = inspect.signature(api.GroundSegmentation.clearance_planes).parameters
    assert list(params) == ["self", "seeds", "max_cells", "order", "nearest", "distance", "out", "on_torch_stream"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[2:])
    assert [f for f in api.ClearanceOutputs.__dataclass_fields__] == ["dist2", "nearest", "distance", "n_occupied"]


class NoLibrary:
    """in place of the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


def test_python_entry_points_refuse_bad_arguments_before_any_library_call(lib):
    import torch

    seg = api.GroundSegmentation()
    seg._L, seg.rows, seg.cols, seg.device = NoLibrary(), 79, 79, 0
    points = torch.zeros((1, 64, 16), dtype=torch.uint8)
    for kw in (dict(order="fortran"), dict(max_cells=-1), dict(max_cells=1.5), dict(min_points=0), dict(min_height=math.nan), dict(max_height=math.nan)):
        with pytest.raises(ValueError):
            seg.clearance_clouds(points, [64], labels=torch.zeros((1, 64), dtype=torch.uint8), **kw)
    host_plane = torch.zeros((1, 79, 79), dtype=torch.int32)
    for args, kw in (((host_plane,), dict(order="fortran")), ((host_plane,), dict(max_cells=-2)), ((host_plane,), {}),  # (not on the device)
                     ((None,), {}), ((np.zeros((1, 79, 79), np.int32),), {})):
        with pytest.raises(ValueError):
            seg.clearance_planes(*args, **kw)


# ---------------------------------------------------------------- the expectation against scipy.ndimage.distance_transform_edt

@pytest.fixture(scope="module")
def expected_row():
    """(patterns, expected_clearance(.., 0, "row")) of every pattern, once"""
    pats = clearance_ref.patterns(79, 79)
    return pats, {name: clearance_ref.expected_clearance(occ, 0, "row", 0.33) for name, occ in pats.items()}


def test_reference_equals_scipy_on_every_pattern(expected_row):
    ndimage = pytest.importorskip("scipy.ndimage")
    pats, want = expected_row
    assert len(pats) == 14 + 7 and list(pats)[14:] == ["corner_00", "corner_0c", "corner_r0", "corner_rc", "four_corners", "pairs", "border_lines"]
    rr, cc = np.mgrid[0:79, 0:79]
    for name, occ in pats.items():
        dist2, nearest, distance, n_occ = want[name]
        assert n_occ == int(occ.sum())
        if not occ.any():
            assert np.all(dist2 == clearance_ref.NONE) and np.all(nearest == -1) and np.all(distance == clearance_ref.INF_BITS)
            continue
        edt = ndimage.distance_transform_edt(~occ)
        assert np.array_equal(np.rint(edt * edt).astype(np.int64), dist2), name
        nr, nc = nearest // 79, nearest % 79
        assert occ[nr, nc].all(), name                                   # the cell `nearest` names is occupied ...
        assert np.array_equal((rr - nr) ** 2 + (cc - nc) ** 2, dist2), name  # ... and lies at exactly dist2
        assert np.array_equal(nearest[occ], (rr * 79 + cc)[occ]) and np.all(dist2[occ] == 0), name
        assert np.array_equal(distance.view(np.float32), np.sqrt(dist2.astype(np.float32)) * np.float32(0.33)), name


@pytest.mark.parametrize("order", ["row", "col"])
def test_tie_rule_against_a_loop_per_cell(expected_row, order):
    pats, want = expected_row
    ties = clearance_ref.tie_patterns(79, 79)
    picks = {"four_corners": [(39, 39), (39, 10), (10, 39), (0, 39), (39, 78), (40, 39), (39, 40)],
             "pairs": [(10, 23), (34, 50), (58, 13), (9, 23), (34, 49), (57, 14), (59, 12)],
             "border_lines": [(5, 73), (1, 77), (40, 38), (78, 0)]}
    for name, occ in ties.items():
        if order == "row":
            got = want[name]
        else:
            got = clearance_ref.expected_clearance(occ, 0, "col", 0.33)
        rng = np.random.default_rng(5900)
        cells = picks.get(name, []) + [tuple(int(v) for v in rng.integers(0, 79, 2)) for _ in range(12)]
        for r, c in cells:
            d2, nr, nc = clearance_ref.nearest_by_loop(occ, r, c)
            assert int(got[0][r, c]) == d2, (name, r, c)
            assert int(got[1][r, c]) == clearance_ref.cluster_ref.linear_index(nr, nc, 79, 79, order), (name, r, c)
    four = want["four_corners"]
    assert int(four[0][39, 39]) == 2 * 39 * 39 and int(four[1][39, 39]) == 0  # the four-way tie goes to (0, 0)
    assert int(want["pairs"][1][10, 23]) == 10 * 79 + 20 and int(want["pairs"][1][34, 50]) == 30 * 79 + 50 and int(want["pairs"][1][58, 13]) == 55 * 79 + 10


def test_radius_changes_nothing_inside_it(expected_row):
    pats, want = expected_row
    for name in ("random_30", "pairs", "borders", "four_corners"):
        free = want[name]
        for R in (1, 7, 200):
            dist2, nearest, distance, n_occ = clearance_ref.expected_clearance(pats[name], R, "row", 0.33)
            inside = free[0] <= R * R
            assert n_occ == free[3]
            assert np.array_equal(dist2[inside], free[0][inside]) and np.array_equal(nearest[inside], free[1][inside]) and np.array_equal(distance[inside], free[2][inside])
            assert np.all(dist2[~inside] == clearance_ref.NONE) and np.all(nearest[~inside] == -1) and np.all(distance[~inside] == clearance_ref.INF_BITS)
        assert (want[name][0] > 49).any() or name == "random_30"
