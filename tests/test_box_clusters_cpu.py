"""gg_box_clusters without a GPU: the entry point is declared, exported, bound and reachable, the ctypes mirrors have the layout the C
compiler gives the two structs, and a null context is refused before the device is touched.  And the expectation of the GPU tests
(tests/box_ref.py) is held without the code under test: against a plain per-point loop, against answers fixed by hand, on L-shapes of a
known heading and against its invariants; BoxOutputs.metric against a float64 computation of the same rectangle."""
import ctypes as C
import inspect
import math
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
from tests import box_ref  # noqa: E402
from tests.box_ref import AREA, EDGE  # noqa: E402

BOX_FIELDS = list(box_ref.FIELDS)
CALL_FIELDS = ["n", "first_slot", "slots", "point_format", "d_points", "cloud_stride", "n_points", "transforms", "d_point_cluster", "d_n_clusters",
               "rotations", "n_rotations", "criterion", "max_clusters", "d_boxes", "d_costs"]
QUARTER = [k * (math.pi / 2) / 16 for k in range(16)]  # sixteen headings over [0, 90 degrees)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- 1. the boundary

def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "groundgrid_hip.h")).read()
    for line in ("#define GG_HAS_BOX_CLUSTERS 1", "#define GG_BOX_UNIT 16", "#define GG_BOX_MAX_HEADINGS 32", "#define GG_BOX_MAX_CLUSTERS 4096"):
        assert re.search("^" + line + "$", header, re.M), line
    assert "int gg_box_clusters(gg_context *ctx, const gg_cluster_boxes *x, void *stream);" in header
    assert "gg_box_clusters" in _lib.SYMBOLS and _lib.GG_HAS_BOX_CLUSTERS == 1
    assert (_lib.GG_BOX_UNIT, _lib.GG_BOX_MAX_HEADINGS, _lib.GG_BOX_MAX_CLUSTERS, _lib.GG_BOX_AREA, _lib.GG_BOX_EDGE) == (16, 32, 4096, 0, 1)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT gg_box_clusters\b", out)
    assert lib.gg_abi_version() == 6
    assert lib.gg_box_clusters(None, None, None) == -1  # a null context, before the device is touched
    x = _lib.GGClusterBoxes()
    assert lib.gg_box_clusters(None, C.byref(x), None) == -1
    internal = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    assert f"BOX_LDS_BUDGET = {_lib.GG_BOX_LDS_BUDGET // 1024} * 1024" in internal and "BOX_PAIR_BYTES = 24" in internal
    assert _lib.box_slab_clusters(32, 4096) == 191 and _lib.box_slab_clusters(16, 4096) == 380 and _lib.box_slab_clusters(16, 256) == 256
    assert "k24_boxes.hip" in open(os.path.join(ROOT, "groundgrid_amd", "csrc", "Makefile")).read()


def test_struct_mirrors_match_the_header():
    assert [n for n, _ in _lib.GGBox._fields_] == BOX_FIELDS and [n for n, _ in _lib.GGClusterBoxes._fields_] == CALL_FIELDS
    args = ["sizeof(gg_box)", "sizeof(gg_cluster_boxes)"] + [f"offsetof(gg_box, {m})" for m in BOX_FIELDS] + [f"offsetof(gg_cluster_boxes, {m})" for m in CALL_FIELDS]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "groundgrid_hip.h"\nint main(void){ size_t v[] = {' + ", ".join(args) + \
           '}; for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]); ' \
           'printf("%d %d %d %d %d\\n", GG_BOX_UNIT, GG_BOX_MAX_HEADINGS, GG_BOX_MAX_CLUSTERS, GG_BOX_AREA, GG_BOX_EDGE); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "t")], text=True).split()))
    want = [C.sizeof(_lib.GGBox), C.sizeof(_lib.GGClusterBoxes)] + [getattr(_lib.GGBox, m).offset for m in BOX_FIELDS] + \
           [getattr(_lib.GGClusterBoxes, m).offset for m in CALL_FIELDS] + [16, 32, 4096, 0, 1]
    assert vals == want and vals[0] == 32
    assert api.BOX_DTYPE == box_ref.BOX_DTYPE and api.BOX_DTYPE.itemsize == 32 and list(api.BOX_DTYPE.names) == BOX_FIELDS


def test_python_method_has_the_documented_signature():
    sig = inspect.signature(api.GroundSegmentation.box_clusters)
    names = list(sig.parameters)
    assert names == ["self", "points", "n_points", "point_cluster", "n_clusters", "rotations", "transforms", "slots", "first_slot", "criterion",
                     "max_clusters", "costs", "out", "on_torch_stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["transforms"], d["slots"], d["first_slot"], d["criterion"], d["max_clusters"], d["costs"], d["out"], d["on_torch_stream"]) == \
           (None, None, 0, "edge", 256, False, None, False)
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[6:])
    assert {"boxes", "costs"} <= set(api.BoxOutputs.__dataclass_fields__)
    assert np.array_equal(api.rotation_table(QUARTER), box_ref.rotation_table(QUARTER))


# ---------------------------------------------------------------- 2. two formulations

def random_case(rng):
    side = int(rng.choice([23, 41, 79]))
    res = float(np.float32(rng.choice([0.33, 0.25, 1.0])))
    pos = (float(rng.normal(0, 30)), float(rng.normal(0, 30)))
    n = int(rng.integers(0, 400))
    K = int(rng.choice([1, 2, 5, 16, 32]))
    M = int(rng.choice([1, 3, 16, 64]))
    n_clusters = int(rng.choice([-3, 0, 1, 2, 7, 40, 1000]))
    half = 0.5 * side * res
    px = (pos[0] + rng.uniform(-1.2 * half, 1.2 * half, n)).astype(np.float32)
    py = (pos[1] + rng.uniform(-1.2 * half, 1.2 * half, n)).astype(np.float32)
    ids = rng.integers(-2, min(max(n_clusters, 1), M) + 3, n).astype(np.int32)  # (a few ids below 0 and behind min(n_clusters, M))
    if n > 8:
        ids[:3] = (np.iinfo(np.int32).min, -1, np.iinfo(np.int32).max)
        px[3], py[4], px[5] = np.nan, np.inf, -np.inf
    rot = box_ref.rotation_table(rng.uniform(-math.pi, math.pi, K))
    inside = box_ref.inside_map(px, py, pos, res, side, side)
    return px, py, ids, n_clusters, pos, res, rot, int(rng.integers(0, 2)), M, inside


def test_two_formulations_agree_on_random_cases():
    rng = np.random.default_rng(2401)
    with_points = multi = 0
    for _ in range(120):
        case = random_case(rng)
        a, b = box_ref.expected_boxes(*case), box_ref.expected_boxes_loop(*case)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), case[3:9]
        Mi, rec, costs = a
        assert Mi == min(max(case[3], 0), case[8]) and rec.shape == (Mi, 8) and costs.shape == (Mi, len(case[6]))
        empty = rec[:, 0] < 0
        assert not rec[empty, 1:].any() and np.all(costs[empty] == box_ref.NO_COST) and np.all(rec[~empty, 1] > 0)
        with_points += int((~empty).sum())
        multi += int((rec[:, 1] > 2).sum())
    assert with_points > 300 and multi > 100


# ---------------------------------------------------------------- 3. known answers

def units(ux, uy):
    """float32 points whose units are (ux, uy) under resolution 1.0 and position (0, 0): the centre of the unit"""
    return ((np.asarray(ux) + 0.5) / 16.0).astype(np.float32), ((np.asarray(uy) + 0.5) / 16.0).astype(np.float32)


def boxes_of(ux, uy, ids, rot, criterion, n_clusters=None, M=8):
    px, py = units(ux, uy)
    ids = np.asarray(ids, dtype=np.int32)
    n_clusters = int(ids.max()) + 1 if n_clusters is None else n_clusters
    args = (px, py, ids, n_clusters, (0.0, 0.0), 1.0, rot, criterion, M, np.ones(len(ids), bool))
    a, b = box_ref.expected_boxes(*args), box_ref.expected_boxes_loop(*args)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    return a


def test_known_answers():
    Q = box_ref.Q14
    axis = np.array([[Q, 0]], dtype=np.int32)
    # the six points of an axis-aligned 3 x 2 block, one unit apart
    ux, uy = np.meshgrid(np.arange(10, 13), np.arange(-4, -2), indexing="ij")
    for crit, cost in ((AREA, (2 * Q) * (1 * Q)), (EDGE, 0)):  # (every point of a 3 x 2 block lies on an edge)
        Mi, rec, costs = boxes_of(ux.ravel(), uy.ravel(), np.zeros(6), axis, crit)
        assert Mi == 1 and list(rec[0]) == [0, 6, 10 * Q, 12 * Q, -4 * Q, -3 * Q, cost & 0xFFFFFFFF, cost >> 32] and int(costs[0, 0]) == cost
    # ... and a 5 x 3 block: its one inner row of three points lies 1, 1, 1 units from the nearest edge; the area is 4 x 2
    ux, uy = np.meshgrid(np.arange(5), np.arange(3), indexing="ij")
    Mi, rec, costs = boxes_of(ux.ravel(), uy.ravel(), np.zeros(15), axis, EDGE)
    assert int(costs[0, 0]) == 3 * Q and list(rec[0, :6]) == [0, 15, 0, 4 * Q, 0, 2 * Q]
    assert int(boxes_of(ux.ravel(), uy.ravel(), np.zeros(15), axis, AREA)[2][0, 0]) == 8 * Q * Q
    # a single point: heading 0 and cost 0 whatever the table holds
    table = box_ref.rotation_table([0.7, 0.0, 0.3])
    for crit in (AREA, EDGE):
        Mi, rec, costs = boxes_of([7], [-9], [0], table, crit)
        cq, sq = int(table[0, 0]), int(table[0, 1])
        a, b = 7 * cq - 9 * sq, -9 * cq - 7 * sq
        assert list(rec[0]) == [0, 1, a, a, b, b, 0, 0] and not costs.any()
    # two points on a diagonal, K = 2 at 0 and 45 degrees: the diagonal heading has no width, so its area is 0 and it wins under AREA; under
    # EDGE both points lie on an edge at either heading, 0 == 0, and the tie goes to the earlier entry
    d = box_ref.rotation_table([0.0, math.pi / 4])
    assert d.tolist() == [[16384, 0], [11585, 11585]]
    Mi, rec, costs = boxes_of([0, 8], [0, 8], [0, 0], d, AREA)
    assert costs[0].tolist() == [(8 * Q) ** 2, 0] and list(rec[0]) == [1, 2, 0, 16 * 11585, 0, 0, 0, 0]
    Mi, rec, costs = boxes_of([0, 8], [0, 8], [0, 0], d, EDGE)
    assert costs[0].tolist() == [0, 0] and list(rec[0]) == [0, 2, 0, 8 * Q, 0, 8 * Q, 0, 0]
    # ... with the table order swapped the tie goes to 45 degrees, which is now first
    Mi, rec, costs = boxes_of([0, 8], [0, 8], [0, 0], d[::-1].copy(), EDGE)
    assert rec[0, 0] == 0 and list(rec[0, 2:6]) == [0, 16 * 11585, 0, 0]
    # a cluster that no point carries between two that are; ids beyond n_clusters select nothing; a cost with a high word
    Mi, rec, costs = boxes_of([0, 1, 5, 40000, -40000], [0, 0, 5, 40000, -40000], [0, 0, 7, 2, 2], axis, AREA, n_clusters=3)
    assert Mi == 3 and rec[1].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and int(costs[1, 0]) == 2 ** 64 - 1 and rec[0, 1] == 2 and rec[2, 1] == 2
    big = (80000 * Q) ** 2
    assert int(costs[2, 0]) == big and (int(rec[2, 6]) & 0xFFFFFFFF, int(rec[2, 7])) == (big & 0xFFFFFFFF, big >> 32) and big >> 32 > 0


# ---------------------------------------------------------------- 4. the L-shape of a car

def l_shape(rng, k, length=4.5, width=1.61, centre=(3.0, -7.0), step=0.04):
    """points on two adjacent sides of a length x width rectangle whose long side points along QUARTER[k], seen from one corner"""
    th = QUARTER[k]
    s = np.concatenate([np.stack([np.arange(0.0, length + 1e-9, step), np.zeros(int(length / step + 1e-9) + 1)], 1),
                        np.stack([np.zeros(int(width / step + 1e-9) + 1), np.arange(0.0, width + 1e-9, step)], 1)])
    s -= (0.5 * length, 0.5 * width)
    x = centre[0] + s[:, 0] * math.cos(th) - s[:, 1] * math.sin(th)
    y = centre[1] + s[:, 0] * math.sin(th) + s[:, 1] * math.cos(th)
    order = rng.permutation(len(x))
    return x[order].astype(np.float32), y[order].astype(np.float32)


# Which L-shapes have ONE smallest rectangle.  The hull of an L with sides L and W is a right triangle, and every rectangle that lies on one
# of its three edges has the area L W: between the long side (0) and the hypotenuse (alpha = atan(W / L)) the area of the bounding rectangle
# is L W cos^2 + (W^2 / 2) sin(2 phi), which peaks at alpha / 2 only (sqrt(1 + (W / L)^2) - 1) / 2 above L W -- 3 % for a car of 4.5 x 1.61.
# A candidate that falls into (0, alpha] therefore ties with the true heading up to the quantisation: the known weakness of the area
# criterion on L-shapes, and the reason "edge" is the default.  AREA is held on shapes whose alpha (4.8 degrees for 6.0 x 0.5) is smaller
# than the table's step of 5.625 degrees, so no candidate but the true one lies in [0, alpha]; beyond alpha the area grows like L^2 sin.
# EDGE is held on the car as well: off the true heading the points of the long side leave their edge and the sum grows with every point.
L_SHAPES = [(AREA, 6.0, 0.5), (EDGE, 6.0, 0.5), (EDGE, 4.5, 1.61)]


@pytest.mark.parametrize("criterion,length,width", L_SHAPES)
def test_l_shapes_return_their_heading(criterion, length, width):
    rng = np.random.default_rng(2402)
    rot = box_ref.rotation_table(QUARTER)
    res, pos = float(np.float32(0.33)), (1.25, -2.5)
    assert criterion == EDGE or math.degrees(math.atan2(width, length)) < 90.0 / 16
    for k in range(16):
        px, py = l_shape(rng, k, length, width)
        args = (px, py, np.zeros(len(px), np.int32), 1, pos, res, rot, criterion, 4, np.ones(len(px), bool))
        Mi, rec, costs = box_ref.expected_boxes(*args)
        assert rec[0, 0] == k, (criterion, k, costs[0].tolist())
        assert np.array_equal(rec, box_ref.expected_boxes_loop(*args)[1])
        cx, cy, got_l, got_w, yaw = box_ref.metric_box(rec[0], rot, res, pos)
        assert abs(got_l - length) < 0.05 and abs(got_w - width) < 0.05 and abs(cx - 3.0) < 0.05 and abs(cy + 7.0) < 0.05 and abs(yaw - QUARTER[k]) < 1e-4


# ---------------------------------------------------------------- 5. invariants

def test_projections_lie_inside_the_extents_and_translation_shifts_them():
    rng = np.random.default_rng(2403)
    rot = box_ref.rotation_table(rng.uniform(0, math.pi / 2, 7))
    for crit in (AREA, EDGE):
        for _ in range(20):
            n = int(rng.integers(1, 120))
            ux, uy, ids = rng.integers(-500, 500, n), rng.integers(-500, 500, n), rng.integers(0, 5, n)
            Mi, rec, costs = boxes_of(ux, uy, ids, rot, crit, n_clusters=5)
            a, b = box_ref.projections(ux, uy, rot)
            for k in range(len(rot)):  # the extents at heading k: the record of a call whose table is that heading alone
                _, rk, ck = boxes_of(ux, uy, ids, rot[k: k + 1], crit, n_clusters=5)
                assert np.array_equal(ck[:, 0], costs[:, k])
                for c in np.unique(ids):
                    sel = ids == c
                    assert np.all(a[sel, k] >= rk[c, 2]) and np.all(a[sel, k] <= rk[c, 3]) and np.all(b[sel, k] >= rk[c, 4]) and np.all(b[sel, k] <= rk[c, 5])
                    assert (a[sel, k].min(), a[sel, k].max(), b[sel, k].min(), b[sel, k].max()) == tuple(rk[c, 2:6])
            # a translation by whole units shifts the bounds by the translation's projections and leaves costs and k* alone
            dx, dy = int(rng.integers(-300, 300)), int(rng.integers(-300, 300))
            Mi2, rec2, costs2 = boxes_of(ux + dx, uy + dy, ids, rot, crit, n_clusters=5)
            assert np.array_equal(costs, costs2) and np.array_equal(rec[:, [0, 1, 6, 7]], rec2[:, [0, 1, 6, 7]])
            for c in np.nonzero(rec[:, 0] >= 0)[0]:
                cq, sq = (int(v) for v in rot[rec[c, 0]])
                da, db = dx * cq + dy * sq, dy * cq - dx * sq
                assert (rec2[c, 2:6] - rec[c, 2:6]).tolist() == [da, da, db, db]


def test_overflow_bounds_at_the_largest_map():
    # a side of 4096 cells: |u| <= 8 * 4096 + 1, the extreme table words on both axes
    u = 8 * 4096 + 1
    Q = box_ref.Q14
    assert u * 2 * Q < 2 ** 31
    corners_x, corners_y = [u, u, -u, -u], [u, -u, u, -u]
    res = float(np.float32(0.33))
    px = (np.array(corners_x, dtype=np.float64) * res / 16.0 + 1e-3).astype(np.float32)
    py = (np.array(corners_y, dtype=np.float64) * res / 16.0 + 1e-3).astype(np.float32)
    qx, qy = box_ref.quantise(px, py, (0.0, 0.0), res)
    assert np.abs(qx).max() <= u and np.abs(qy).max() <= u and np.abs(qx).min() >= u - 1
    widest = 0
    for cq, sq in ((Q, Q), (-Q, Q), (Q, -Q), (-Q, -Q), (Q, 0), (0, -Q)):
        rot = np.array([[cq, sq]], dtype=np.int32)
        a, b = box_ref.projections(qx, qy, rot)
        assert np.abs(a).max() < 2 ** 31 and np.abs(b).max() < 2 ** 31
        for crit in (AREA, EDGE):
            args = (px, py, np.zeros(4, np.int32), 1, (0.0, 0.0), res, rot, crit, 1, np.ones(4, bool))
            Mi, rec, costs = box_ref.expected_boxes(*args)
            A, B = int(a.max() - a.min()), int(b.max() - b.min())
            assert A <= 2 ** 31 + 2 ** 16 and B <= 2 ** 31 + 2 ** 16 and A * B < 2 ** 63
            widest = max(widest, A, B)
            assert int(costs[0, 0]) == (A * B if crit == AREA else 0)
            assert np.array_equal(costs, box_ref.expected_boxes_loop(*args)[2])
            assert (int(rec[0, 6]) & 0xFFFFFFFF) | (int(rec[0, 7]) & 0xFFFFFFFF) << 32 == int(costs[0, 0])
    assert widest == 2 ** 31 + 2 ** 16  # (the extent itself does not fit an int32: the 64-bit difference is needed)


# ---------------------------------------------------------------- 6. the metric rectangle

def test_metric_against_a_float64_computation():
    import torch

    rng = np.random.default_rng(2404)
    rot = box_ref.rotation_table(QUARTER)
    res, pos = float(np.float32(0.33)), (12.5, -3.25)
    recs = np.zeros((1, 20, 8), dtype=np.int32)
    recs[0, :, 0] = -1
    for c in range(16):
        px, py = l_shape(rng, c, length=3.0 + 0.1 * c, width=1.0 + 0.05 * c, centre=(pos[0] + c - 8.0, pos[1] + 0.5 * c))
        recs[0, c] = box_ref.expected_boxes(px, py, np.zeros(len(px), np.int32), 1, pos, res, rot, EDGE, 1, np.ones(len(px), bool))[1][0]
        assert recs[0, c, 0] == c
    out = api.BoxOutputs(boxes=torch.from_numpy(recs))
    got = out.metric(0, rot, res, pos)
    assert got.shape == (20, 5) and got.dtype == np.float64 and np.isnan(got[16:]).all()
    for c in range(16):
        want = box_ref.metric_box(recs[0, c], rot, res, pos)
        assert np.allclose(got[c], want, rtol=0, atol=1e-9), (c, got[c], want)
        assert abs(got[c, 0] - (pos[0] + c - 8.0)) < 0.05 and abs(got[c, 1] - (pos[1] + 0.5 * c)) < 0.05
        assert abs(got[c, 2] - (3.0 + 0.1 * c)) < 0.05 and abs(got[c, 3] - (1.0 + 0.05 * c)) < 0.05
    assert recs[0, :16].copy().view(api.BOX_DTYPE)["heading"].ravel().tolist() == list(range(16))
