"""gg_cluster_planes without a GPU: the entry point is declared, exported, bound and reachable, the ctypes mirrors have the layout the C
compiler gives the two structs, and a null context is refused before the device is touched.  And the expectation of the GPU tests
(tests/regions_ref.py) is held without the code under test: against scipy.ndimage.label with a size filter and a sequential relabelling
on every pattern of cluster_ref.patterns(), and against known answers fixed by hand."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, build  # noqa: E402
from tests import cluster_ref, regions_ref  # noqa: E402

REGION_FIELDS = regions_ref.FIELDS
CALL_FIELDS = ["n", "d_seeds", "seed_stride", "lo", "hi", "connectivity", "min_cells", "order", "d_values", "value_stride", "d_cell_cluster",
               "plane_stride", "d_cell_size", "size_stride", "d_heads", "d_regions", "max_regions"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- 1. the boundary

def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "groundgrid_hip.h")).read()
    assert re.search(r"^#define GG_HAS_CLUSTER_PLANES 1$", header, re.M)
    assert re.search(r"^int gg_cluster_planes\(gg_context \*ctx, const gg_plane_clusters \*x, void \*stream\);$", header, re.M)
    assert re.search(r"^#define GG_ABI_VERSION 6$", header, re.M) or lib.gg_abi_version() == 6
    assert "gg_cluster_planes" in _lib.SYMBOLS and _lib.GG_HAS_CLUSTER_PLANES == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT gg_cluster_planes\b", out)
    assert lib.gg_abi_version() == 6
    assert lib.gg_cluster_planes(None, None, None) == -1  # a null context, before the device is touched
    x = _lib.GGPlaneClusters()
    assert lib.gg_cluster_planes(None, C.byref(x), None) == -1
    assert "k26_regions.hip" in open(os.path.join(ROOT, "groundgrid_amd", "csrc", "Makefile")).read()


def test_struct_mirrors_match_the_header():
    assert [n for n, _ in _lib.GGRegion._fields_] == REGION_FIELDS and [n for n, _ in _lib.GGPlaneClusters._fields_] == CALL_FIELDS
    args = ["sizeof(gg_region)", "sizeof(gg_plane_clusters)"] + [f"offsetof(gg_region, {m})" for m in REGION_FIELDS] + \
           [f"offsetof(gg_plane_clusters, {m})" for m in CALL_FIELDS]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "groundgrid_hip.h"\nint main(void){ size_t v[] = {' + ", ".join(args) + \
           '}; for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]); printf("%d\\n", GG_HAS_CLUSTER_PLANES); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "t")], text=True).split()))
    want = [C.sizeof(_lib.GGRegion), C.sizeof(_lib.GGPlaneClusters)] + [getattr(_lib.GGRegion, m).offset for m in REGION_FIELDS] + \
           [getattr(_lib.GGPlaneClusters, m).offset for m in CALL_FIELDS] + [1]
    assert vals == want and vals[0] == 48 == _lib.GG_REGION_BYTES
    assert vals[2:12] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]  # the offsets the header's table names
    assert api.REGION_DTYPE == regions_ref.REGION_DTYPE and api.REGION_DTYPE.itemsize == 48 and list(api.REGION_DTYPE.names) == REGION_FIELDS
    assert [api.REGION_DTYPE.fields[m][1] for m in REGION_FIELDS] == vals[2:12]


def test_python_method_has_the_documented_signature():
    sig = inspect.signature(api.GroundSegmentation.cluster_planes)
    assert list(sig.parameters) == ["self", "seeds", "lo", "hi", "connectivity", "min_cells", "values", "max_regions", "order", "sizes", "out", "on_torch_stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert [d[k] for k in list(sig.parameters)[2:]] == [0, None, 8, 1, None, 256, "row", False, None, False]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for k, p in sig.parameters.items() if k not in ("self", "seeds"))
    assert list(api.RegionOutputs.__dataclass_fields__) == ["cell_cluster", "cell_size", "heads", "regions"]
    assert callable(api.RegionOutputs.centroids) and callable(api.RegionOutputs.table)


# ---------------------------------------------------------------- 2. the reference against scipy

def scipy_regions(member, connectivity, min_cells, order):
    """scipy.ndimage.label, a size filter and a sequential relabelling: (plane, sizes, heads).  scipy numbers in row-major scan order, so
    the column-major numbering is the label of the transposed mask"""
    from scipy import ndimage

    structure = np.ones((3, 3), dtype=int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    lab, n_all = ndimage.label(member if order == "row" else member.T, structure)
    if order == "col":
        lab = lab.T
    size_of = np.bincount(lab.ravel(), minlength=n_all + 1)
    size_of[0] = 0
    sizes = size_of[lab].astype(np.int32)
    plane = np.full(lab.shape, -1, dtype=np.int32)
    k = 0
    for old in range(1, n_all + 1):  # sequential: in scipy's order, which is the order of the smallest linear index
        if size_of[old] >= min_cells:
            plane[lab == old] = k
            k += 1
    return plane, sizes, np.array([k, n_all - k, int(member.sum()), int((plane >= 0).sum())], dtype=np.int32)


@pytest.fixture(scope="module")
def labelled():
    """cluster_ref.label_plane of every pattern, once per (connectivity, order)"""
    pats = cluster_ref.patterns()
    return pats, {(name, conn, order): cluster_ref.label_plane(occ, conn, order) for name, occ in pats.items() for conn in (4, 8) for order in ("row", "col")}


@pytest.mark.parametrize("min_cells", [1, 2, 5])
@pytest.mark.parametrize("order", ["row", "col"])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_reference_against_scipy_on_every_pattern(labelled, connectivity, order, min_cells):
    pats, labels = labelled
    assert len(pats) == 14
    for name, occ in pats.items():
        plane, sizes, heads, rec = regions_ref.regions_of_labels(labels[name, connectivity, order], min_cells, order)
        want_plane, want_sizes, want_heads = scipy_regions(occ, connectivity, min_cells, order)
        assert np.array_equal(plane, want_plane) and np.array_equal(sizes, want_sizes) and np.array_equal(heads, want_heads), name
        # the records against the plane, cell by cell
        rows, cols = occ.shape
        assert len(rec) == heads[0]
        for k in range(0, len(rec), max(1, len(rec) // 7)):
            rr, cc = np.nonzero(plane == k)
            L = cluster_ref.linear_index(rr, cc, rows, cols, order)
            assert tuple(rec[k])[:6] == (rr.size, rr.min(), rr.max(), cc.min(), cc.max(), L.min()), (name, k)
            assert (rec[k]["sum_row"], rec[k]["sum_col"], rec[k]["value_min"], rec[k]["value_cell"]) == (rr.sum(), cc.sum(), regions_ref.INT32_MAX, -1)
        assert (np.diff(rec["first_cell"]) > 0).all()  # numbered by ascending smallest L


# ---------------------------------------------------------------- 3. known answers

def test_checkerboard_at_connectivity_4_with_min_cells_2_keeps_nothing():
    occ = cluster_ref.patterns()["checkerboard"]
    seeds = np.where(occ, 0, -1)
    for order in ("row", "col"):
        plane, sizes, heads, rec = regions_ref.expected_regions(seeds, connectivity=4, min_cells=2, order=order)
        assert heads.tolist() == [0, 3121, 3121, 0] and len(rec) == 0  # every member is a component of its own, and dropped
        assert (plane == -1).all() and np.array_equal(sizes, occ.astype(np.int32))
    plane, sizes, heads, rec = regions_ref.expected_regions(seeds, connectivity=8, min_cells=2)
    assert heads.tolist() == [1, 0, 3121, 3121] and rec["cells"].tolist() == [3121] and (sizes[occ] == 3121).all()


def test_constant_value_plane_gives_the_first_cell():
    for name, occ in cluster_ref.patterns().items():
        for order in ("row", "col"):
            _, _, heads, rec = regions_ref.expected_regions(np.where(occ, 7, -3), lo=7, hi=7, connectivity=4, order=order, values=np.full(occ.shape, -5))
            assert np.array_equal(rec["value_cell"], rec["first_cell"]) and (rec["value_min"] == -5).all(), name


def test_range_and_value_minimum_by_hand():
    seeds = np.array([[1, 1, -1, 0],
                      [-1, -1, -1, 0],
                      [1, -1, 1, 1]])
    values = np.array([[5, 3, 0, 9],
                       [0, 0, 0, -4],
                       [2, 0, -4, -4]])
    plane, sizes, heads, rec = regions_ref.expected_regions(seeds, lo=0, connectivity=4, min_cells=2, values=values)
    assert plane.tolist() == [[0, 0, -1, 1], [-1, -1, -1, 1], [-1, -1, 1, 1]]
    assert sizes.tolist() == [[2, 2, 0, 4], [0, 0, 0, 4], [1, 0, 4, 4]] and heads.tolist() == [2, 1, 7, 6]
    assert rec["value_min"].tolist() == [3, -4] and rec["value_cell"].tolist() == [1, 7]  # (-4 at L = 7, 10 and 11: the smallest)
    assert rec["sum_row"].tolist() == [0, 5] and rec["sum_col"].tolist() == [1, 11] and rec["first_cell"].tolist() == [0, 3]
    plane, _, heads, rec = regions_ref.expected_regions(seeds, lo=1, hi=1, connectivity=8, order="col", values=values)
    assert plane.tolist() == [[0, 0, -1, -1], [-1, -1, -1, -1], [1, -1, 2, 2]] and heads.tolist() == [3, 0, 5, 5]
    assert rec["first_cell"].tolist() == [0, 2, 8] and rec["value_cell"].tolist() == [3, 2, 8] and rec["value_min"].tolist() == [3, 2, -4]
    assert regions_ref.words_of(rec).shape == (3, 12)
