"""gg_cluster_clouds without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirrors have the
layout the C compiler gives the structs, the ABI version and the neighbouring structs are what they were, and a null context is refused
before the device is touched.  And the expectation of the GPU tests (tests/cluster_ref.py) is held against scipy.ndimage.label on every
pattern those tests run, without the code under test."""
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
from tests import cluster_ref  # noqa: E402

CLUSTER_FIELDS = ["cells", "points", "row_min", "row_max", "col_min", "col_max", "height_max", "first_cell"]
CLOUD_FIELDS = ["n", "first_slot", "slots", "point_format", "d_points", "cloud_stride", "n_points", "transforms", "d_labels", "d_label_masks",
                "min_points", "min_height", "max_height", "connectivity", "order", "d_cell_cluster", "plane_stride", "d_point_cluster", "d_n_clusters",
                "d_clusters", "max_clusters"]


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
    assert "gg_cluster_clouds" in _lib.SYMBOLS
    assert hasattr(lib, "gg_cluster_clouds")
    assert len(lib.gg_cluster_clouds.argtypes) == 3


def test_field_lists_of_both_structs():
    assert [f[0] for f in _lib.GGCluster._fields_] == CLUSTER_FIELDS == cluster_ref.FIELDS
    assert [f[0] for f in _lib.GGCloudClusters._fields_] == CLOUD_FIELDS
    assert CLOUD_FIELDS[:10] == [f[0] for f in _lib.GGCloudRaster._fields_][:10]  # the ten leading members of gg_cloud_raster
    assert list(api.CLUSTER_DTYPE.names) == CLUSTER_FIELDS and api.CLUSTER_DTYPE.itemsize == 32


def test_struct_layouts_equal_the_ctypes_mirrors(lib):
    lines = ['printf("%zu\\n", sizeof(gg_cluster));']
    lines += [f'printf("%zu\\n", offsetof(gg_cluster, {k}));' for k in CLUSTER_FIELDS]
    lines += ['printf("%zu\\n", sizeof(gg_cloud_clusters));']
    lines += [f'printf("%zu\\n", offsetof(gg_cloud_clusters, {k}));' for k in CLOUD_FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    got = [int(v) for v in out.split()]
    want = [C.sizeof(_lib.GGCluster)] + [getattr(_lib.GGCluster, k).offset for k in CLUSTER_FIELDS]
    want += [C.sizeof(_lib.GGCloudClusters)] + [getattr(_lib.GGCloudClusters, k).offset for k in CLOUD_FIELDS]
    assert got == want
    assert got[0] == 32
    assert [api.CLUSTER_DTYPE.fields[k][1] for k in CLUSTER_FIELDS] == got[1:9]


def test_feature_macro_is_one(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_CLUSTER_CLOUDS) || GG_HAS_CLUSTER_CLOUDS != 1
    #error "GG_HAS_CLUSTER_CLOUDS"
    #endif
    int main(void) { printf("%d\n", GG_HAS_CLUSTER_CLOUDS); return 0; }
    ''')
    assert int(out) == 1


def test_abi_version_and_the_other_structs_are_unchanged(lib):
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { printf("%d %zu %zu %zu\n", GG_ABI_VERSION, sizeof(gg_batch), sizeof(gg_cloud_raster), sizeof(gg_cloud_split)); return 0; }
    ''')
    version, batch, raster, split = (int(v) for v in out.split())
    assert version == 6
    assert batch == C.sizeof(_lib.GGBatch) == 120
    assert raster == C.sizeof(_lib.GGCloudRaster)
    assert split == C.sizeof(_lib.GGCloudSplit)


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <math.h>
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int step(gg_context *ctx, const gg_point16 *d_points, const uint8_t *d_labels, int32_t *d_planes, int32_t *d_ids, int32_t *d_counts, gg_cluster *d_table,
             void *stream) {
        const int32_t slots[2] = {3, 1}, n_points[2] = {1000, 64};
        gg_cloud_clusters x = {0};
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
        x.connectivity = 8;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_cell_cluster = d_planes;
        x.plane_stride = 364 * 364;
        x.d_point_cluster = d_ids;
        x.d_n_clusters = d_counts;
        x.d_clusters = d_table;
        x.max_clusters = 256;
        int rc = gg_cluster_clouds(ctx, &x, stream);
        x.slots = NULL;
        x.first_slot = 4;
        x.d_labels = NULL;
        x.d_label_masks = d_labels;
        x.connectivity = 4;
        x.d_clusters = NULL;
        x.max_clusters = 0;
        return rc + gg_cluster_clouds(ctx, &x, GG_STREAM_DEFAULT);
    }
    int main(void) { return step(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == 2 * GG_ERR_INVALID && sizeof(gg_cluster) == 32 ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGCloudClusters()
    x.n = 1
    assert lib.gg_cluster_clouds(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_cluster_clouds(None, None, None) == -1
    x.n = 0
    assert lib.gg_cluster_clouds(None, C.byref(x), None) == -1


def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.cluster_clouds).parameters
    assert list(params)[:3] == ["self", "points", "n_points"]
    defaults = {"labels": None, "masks": None, "transforms": None, "slots": None, "first_slot": 0, "min_points": 1, "min_height": -math.inf,
                "max_height": math.inf, "connectivity": 8, "max_clusters": 256, "order": "row", "point_clusters": True, "out": None,
                "on_torch_stream": True}
    assert list(params)[3:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert [f for f in api.ClusterOutputs.__dataclass_fields__] == ["cell_cluster", "n_clusters", "clusters", "point_cluster"]
    assert callable(api.ClusterOutputs.table)


# ---------------------------------------------------------------- the expectation against scipy.ndimage.label

STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1], [1, 1, 1], [1, 1, 1]]}
EXPECTED_K = {"empty": (0, 0), "full": (1, 1), "checkerboard": (3121, 1), "spiral": (1, 1), "comb": (1, 1), "comb_t": (1, 1), "u": (1, 1), "w": (1, 1),
              "corner_blocks": (4, 2), "borders": (8, 8), "trap": (4, 4)}  # (connectivity 4, connectivity 8)


@pytest.mark.parametrize("order", ["row", "col"])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_equals_scipy_on_every_pattern(connectivity, order):
    ndimage = pytest.importorskip("scipy.ndimage")
    pats = cluster_ref.patterns(79, 79)
    assert list(pats)[-3:] == ["random_30", "random_45", "random_60"] and len(pats) == 14
    for name, occ in pats.items():
        got = cluster_ref.label_plane(occ, connectivity, order)
        # scipy numbers components by first appearance in raster order: the column-major case is the transposed array
        lab, K = ndimage.label(occ if order == "row" else occ.T, structure=STRUCTURE[connectivity])
        want = (lab if order == "row" else lab.T).astype(np.int32) - 1
        assert np.array_equal(got, want), f"{name} {connectivity} {order}"
        assert int(got.max()) + 1 == K or (K == 0 and not occ.any())
        if name in EXPECTED_K:
            assert K == EXPECTED_K[name][0 if connectivity == 4 else 1], (name, K)
    assert int(pats["full"].sum()) == 6241 and int(pats["spiral"].sum()) > 3000


def test_reference_table_and_point_ids():
    """expected_clusters on a plane small enough to count by hand"""
    rows, cols = 4, 5
    # cells: (0,0) x2, (0,1) x1, (3,4) x3 (two of them NaN heights), (2,2) x1 (below min_points = ... 1: occupied), one point not participating
    pr = np.array([0, 0, 0, 3, 3, 3, 2, 1])
    pc = np.array([0, 0, 1, 4, 4, 4, 2, 1])
    h = np.array([0.5, -0.0, 0.0, np.nan, np.nan, -np.inf, np.nan, 9.0], dtype=np.float32)
    part = np.array([1, 1, 1, 1, 1, 1, 1, 0], dtype=bool)
    plane, K, table, ids = cluster_ref.expected_clusters(rows, cols, pr, pc, h, part, 1, 4, "row")
    assert K == 3 and list(ids) == [0, 0, 0, 2, 2, 2, 1, -1]
    t = table.view(np.int32)
    assert list(t[0, :6]) == [2, 3, 0, 0, 0, 1] and table[0, 6] == np.float32(0.5).view(np.uint32) and t[0, 7] == 0
    assert list(t[1, :6]) == [1, 1, 2, 2, 2, 2] and table[1, 6] == cluster_ref.QUIET_NAN and t[1, 7] == 12
    assert list(t[2, :6]) == [1, 3, 3, 3, 4, 4] and table[2, 6] == np.float32(-np.inf).view(np.uint32) and t[2, 7] == 19
    plane2, K2, table2, ids2 = cluster_ref.expected_clusters(rows, cols, pr, pc, h, part, 2, 8, "col")
    assert K2 == 2 and list(ids2) == [0, 0, -1, 1, 1, 1, -1, -1] and table2.view(np.int32)[1, 7] == 3 + 4 * rows
    assert np.array_equal(cluster_ref.in_band(np.array([0.3, 0.29999998, 2.5, 2.5000002, np.nan, np.inf], np.float32), 0.3, 2.5), [True, False, True, False, True, False])
