"""gg_score_rollouts without a GPU: the entry point is declared, exported, bound and reachable, the ctypes mirror has the layout the C
compiler gives the struct, and a null context is refused before the device is touched.  The expectation of the GPU tests
(tests/rollouts_ref.py) is held without the code under test against records computed by hand -- the rounding of the rotation at exactly
half, the floor of negative sixteenths, the saturation of `total`, the tie rule of the best rollout -- and against its invariants on
the scenes the GPU tests run; api.rollout_arcs against its closed forms and symmetries; the refusals of the Python method that come
before the device is looked at."""
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
from tests import rollouts_ref as ref  # noqa: E402

NONE = ref.NONE
CALL_FIELDS = ["n", "d_mask", "mask_stride", "d_cost", "cost_stride", "d_dist", "dist_stride", "plane_stride", "d_clear", "clear_stride", "n_headings",
               "starts", "rotations", "frame", "d_table", "table_stride", "n_rollouts", "n_steps", "cost_max", "reach", "order", "d_records",
               "record_stride", "d_best"]
CONSTANTS = ["GG_HAS_SCORE_ROLLOUTS", "GG_ROLLOUTS_MAX", "GG_ROLLOUTS_MAX_STEPS", "GG_ROLLOUTS_MAX_REACH", "GG_ROLLOUTS_RECORD_WORDS",
             "GG_ROLLOUTS_RELATIVE", "GG_ROLLOUTS_ABSOLUTE"]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


# ---------------------------------------------------------------- 1. the boundary

def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "groundgrid_hip.h")).read()
    for line in ("#define GG_HAS_SCORE_ROLLOUTS 1", "#define GG_ROLLOUTS_MAX 65536", "#define GG_ROLLOUTS_MAX_STEPS 128", "#define GG_ROLLOUTS_MAX_REACH 63"):
        assert re.search("^" + line + "$", header, re.M), line
    assert "int gg_score_rollouts(gg_context *ctx, const gg_rollouts *x, void *stream);" in header
    assert "gg_score_rollouts" in _lib.SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT gg_score_rollouts\b", out)
    assert lib.gg_abi_version() == 6
    assert lib.gg_score_rollouts(None, None, None) == -1  # a null context, before the device is touched
    x = _lib.GGRollouts()
    assert lib.gg_score_rollouts(None, C.byref(x), None) == -1
    assert "k25_rollouts.hip" in open(os.path.join(ROOT, "groundgrid_amd", "csrc", "Makefile")).read()


def test_a_c_program_prints_the_macro_the_size_and_the_constants(lib):
    assert [n for n, _ in _lib.GGRollouts._fields_] == CALL_FIELDS
    args = ["sizeof(gg_rollouts)"] + [f"offsetof(gg_rollouts, {m})" for m in CALL_FIELDS]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "groundgrid_hip.h"\nint main(void){ size_t v[] = {' + ", ".join(args) + \
           '}; for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%zu ", v[i]); ' \
           'printf("' + " ".join(["%d"] * (len(CONSTANTS) + 1)) + '\\n", ' + ", ".join(CONSTANTS) + ', GG_ABI_VERSION); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        vals = list(map(int, subprocess.check_output([os.path.join(d, "t")], text=True).split()))
    want = [C.sizeof(_lib.GGRollouts)] + [getattr(_lib.GGRollouts, m).offset for m in CALL_FIELDS] + [getattr(_lib, c) for c in CONSTANTS] + [6]
    assert vals == want
    assert [getattr(_lib, c) for c in CONSTANTS] == [1, 65536, 128, 63, 8, 0, 1]
    assert lib.gg_abi_version() == 6
    assert api.ROLLOUT_DTYPE.itemsize == 32 and list(api.ROLLOUT_DTYPE.names) == list(ref.FIELDS)
    assert (ref.NONE, ref.UNIT, ref.RELATIVE, ref.ABSOLUTE) == (_lib.GG_ROUTE_NONE, _lib.GG_MATCH_UNIT, _lib.GG_ROLLOUTS_RELATIVE, _lib.GG_ROLLOUTS_ABSOLUTE)


def test_python_method_has_the_documented_signature():
    sig = inspect.signature(api.GroundSegmentation.score_rollouts)
    names = list(sig.parameters)
    assert names == ["self", "mask", "table", "starts", "rotations", "relative", "cost", "dist", "clear", "cost_max", "reach", "order", "step_major",
                     "best", "out", "on_torch_stream", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert [d[k] for k in names[4:]] == [None, True, None, None, None, 252, 0, "row", False, True, None, False, None]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[4:])
    assert {"records", "best"} <= set(api.RolloutOutputs.__dataclass_fields__)
    assert list(inspect.signature(api.rollout_arcs).parameters) == ["rotations", "speeds", "turns", "steps", "unit"]
    assert np.array_equal(api.rotation_table(2.0 * np.pi * np.arange(6) / 6), ref.rotations_of(6))


# ---------------------------------------------------------------- 2. the reference against records computed by hand

def all_open(side, K):
    return np.full((1, side, side), (1 << K) - 1, np.int64).astype(np.uint32).view(np.int32)


def test_the_rotation_rounds_half_away_from_zero():
    """K = 6: heading 1 is (8192, 14189), so an offset of one unit forward is exactly half a unit along the rows.  Start (95, 80, 1) on an
    8 x 8 map, w = 1, clear(r, c) = 100 - (8 r + c).
      p0: (1, 0, 0, 3): A = 8192 -> 1, B = 14189 -> 1: (96, 81) = cell (6, 5), k 1.  (-3, 0, -1, 2): A = -24576 -> -2 (1.5 away from
          zero), B = -42567 -> -3 (2.598): (93, 77) = cell (5, 4), k 0.  steps 2, cost 5, end 44, clear min(47, 56).
      p1: (0, 1, 7, 4): A = -14189 -> -1, B = 8192 -> 1: (94, 81) = cell (5, 5), k = 8 mod 6 = 2; then s = 0: len 1.
      p2: s = 0 at once: len 0, complete, the end is the start state (cell 45, k 1), total 0 -- the best."""
    assert [ref.rha(v) for v in (8192, -8192, 8191, -8191, 24576, -24576, 0)] == [1, -1, 0, 0, 2, -2, 0]
    rot = ref.rotations_of(6)
    assert rot[1].tolist() == [8192, 14189]
    table = np.zeros((2, 3, 4), np.int32)
    table[0, 0], table[1, 0] = (1, 0, 0, 3), (-3, 0, -1, 2)
    table[0, 1], table[1, 1] = (0, 1, 7, 4), (9, 9, 9, 0)
    table[0, 2], table[1, 2] = (5, 5, 5, 0), (1, 1, 1, 1)
    clear = (100 - np.arange(64).reshape(1, 8, 8)).astype(np.int32)
    got = ref.expected_rollouts(table, [(95, 80, 1)], 6, ref.RELATIVE, rot, all_open(8, 6), clears=clear)
    assert got["records"][0].tolist() == [[2, 2, 5, 44, 0, 0, 47, 5], [1, 1, 4, 45, 2, 0, 55, 4], [0, 0, 0, 45, 1, 0, NONE, 0]]
    assert got["best"][0].tolist() == [2, 0, 3, 3]


def test_negative_sixteenths_floor_to_the_cell_outside():
    """Absolute frame, K = 1: (-1, 8) is row floor(-1 / 16) = -1, outside -- a division that truncates would call it row 0.  (8, -16) is
    column -1.  (0, 0) with dk = -5 is cell (0, 0), heading -5 mod 1 = 0.  (127, 127) is cell (7, 7).  The same from a relative start at
    (0, 0): one unit backwards leaves the map."""
    table = np.array([[(-1, 8, 0, 1), (8, -16, 0, 1), (0, 0, -5, 1), (127, 127, 3, 2)]], np.int32)
    got = ref.expected_rollouts(table, [(8, 8, 0)], 1, ref.ABSOLUTE, None, all_open(8, 1))
    out = [0, 1, 0, 0, 0, NONE, NONE, NONE]
    assert got["records"][0].tolist() == [out, out, [1, 1, 1, 0, 0, 0, NONE, 1], [1, 1, 2, 63, 0, 0, NONE, 2]]
    assert got["best"][0].tolist() == [2, 1, 2, 2]
    rel = ref.expected_rollouts(np.array([[(-1, 0, 0, 1), (0, -1, 0, 1), (0, 0, 0, 1)]], np.int32), [(0, 0, 0)], 1, ref.RELATIVE, [(16384, 0)], all_open(8, 1))
    assert rel["records"][0][:, 0].tolist() == [0, 0, 1]
    col = ref.expected_rollouts(table, [(8, 8, 0)], 1, ref.ABSOLUTE, None, all_open(8, 1), order="col")
    assert np.array_equal(col["records"], got["records"])  # (cells 0 and 63 are their own transposes; the next test has cells that are not)


def test_total_saturates_unreached_and_negative_togo_do_not_score_and_ties_go_to_the_smallest_p():
    """K = 1, w = min(300, 252) = 252 everywhere.  D is 2^31 - 2 at (1, 1): cost + togo saturates at 2^31 - 2, which is a score.  D is
    GG_ROUTE_NONE at (2, 2) and -1 at (3, 3): complete, not scored.  D(4, 4) = 10 reached with s = 2 and D(4, 5) = 262 with s = 1 both
    total 514: the best is the smaller p."""
    dist = np.zeros((1, 1, 8, 8), np.int32)
    dist[0, 0, 1, 1], dist[0, 0, 2, 2], dist[0, 0, 3, 3], dist[0, 0, 4, 4], dist[0, 0, 4, 5] = NONE - 1, NONE, -1, 10, 262
    cost = np.full((1, 8, 8), 300, np.int32)
    centre = lambda r, c, s: (16 * r + 8, 16 * c + 8, 0, s)
    table = np.array([[centre(1, 1, 1), centre(2, 2, 1), centre(3, 3, 1), centre(4, 4, 2), centre(4, 5, 1)]], np.int32)
    got = ref.expected_rollouts(table, [(0, 0, 0)], 1, ref.ABSOLUTE, None, all_open(8, 1), costs=cost, dists=dist)
    assert got["records"][0].tolist() == [[1, 1, 252, 9, 0, NONE - 1, NONE, NONE - 1], [1, 1, 252, 18, 0, NONE, NONE, NONE], [1, 1, 252, 27, 0, -1, NONE, NONE],
                                          [1, 1, 504, 36, 0, 10, NONE, 514], [1, 1, 252, 37, 0, 262, NONE, 514]]
    assert got["best"][0].tolist() == [3, 514, 5, 3]
    col = ref.expected_rollouts(table, [(0, 0, 0)], 1, ref.ABSOLUTE, None, all_open(8, 1), costs=cost, dists=dist, order="col")
    assert col["records"][0][:, 3].tolist() == [9, 18, 27, 36, 44]  # (4, 5) is 4 + 5 * 8 column-major
    assert col["best"][0].tolist() == [3, 514, 5, 3]


def test_a_blocked_pose_ends_the_steps_but_not_the_length_and_reach_is_a_square():
    """One rollout of four steps along a row; the third cell lacks the heading: steps 2, len 4, not complete.  With reach 1 from the
    start's cell the second pose (two columns away) is already out."""
    mask = all_open(8, 2).copy()
    mask[0, 2, 5] = 1  # heading 0 only
    table = np.array([[(40, 16 * c + 8, 1, 1)] for c in (3, 4, 5, 6)], np.int32)  # [T = 4, P = 1]
    got = ref.expected_rollouts(table, [(40, 40, 0)], 2, ref.ABSOLUTE, None, mask)
    assert got["records"][0].tolist() == [[2, 4, 2, 2 * 8 + 4, 1, NONE, NONE, NONE]] and got["best"][0].tolist() == [-1, NONE, 0, 0]
    got = ref.expected_rollouts(table, [(40, 40, 0)], 2, ref.ABSOLUTE, None, mask, reach=1)
    assert got["records"][0].tolist() == [[1, 4, 1, 2 * 8 + 3, 1, NONE, NONE, NONE]]
    none = ref.expected_rollouts(table, [(-1, 7, 7)], 2, ref.ABSOLUTE, None, mask)
    assert none["records"][0].tolist() == [list(ref.NO_START)] and none["best"][0].tolist() == [-1, NONE, 0, 0]


@pytest.mark.parametrize("frame", [ref.RELATIVE, ref.ABSOLUTE])
def test_the_scenes_of_the_gpu_tests_hold_every_class(frame):
    """the random scenes mix what the contract distinguishes: complete and cut rollouts, early ends and empty rollouts, poses off every side
    of the map, rollouts a reach stops, scored and unscored ends; and the garbage table scores without an error"""
    side, K, P, T = 41, 8, 1025, 33
    rot = ref.rotations_of(K)
    masks, costs, clears, dists = ref.random_planes(side, K, 3, n=2)
    table = ref.mixed_table(P, T, K, side, 1, frame)
    starts = ref.sub_cell_starts(2, side, K, 2)
    assert set(starts[:, 0] % 16) | set(starts[:, 1] % 16) == {0, 8, 15}
    assert table[..., 2].min() < 0 and table[..., 2].max() >= K
    wide = ref.expected_rollouts(table, starts, K, frame, rot, masks, costs, dists, clears)
    near = ref.expected_rollouts(table, starts, K, frame, rot, masks, costs, dists, clears, reach=5)
    for got in (wide, near):
        rec = got["records"]
        steps, length, total = rec[..., 0], rec[..., 1], rec[..., 7]
        assert (steps <= length).all() and (length <= T).all()
        complete = steps == length
        assert (complete & (length == T)).any() and (complete & (length == 0)).any() and (complete & (length > 0) & (length < T)).any() and (~complete).any()
        assert (total[~complete] == NONE).all() and (total[complete] != NONE).any() and (total[complete] == NONE).any()
        assert (rec[..., 6][steps == 0] == NONE).all()
        for i in range(2):
            scored = np.flatnonzero(total[i] != NONE)
            assert got["best"][i].tolist() == [scored[np.argmin(total[i][scored])], total[i][scored].min(), complete[i].sum(), len(scored)]
    assert (near["records"][..., 0] <= wide["records"][..., 0]).all() and (near["records"][..., 0] < wide["records"][..., 0]).any()
    garbage = ref.garbage_table(257, 5, 4)
    assert {ref.I32_MIN, ref.I32_MAX} <= set(garbage[..., 0].ravel()) & set(garbage[..., 1].ravel()) & set(garbage[..., 2].ravel())
    got = ref.expected_rollouts(garbage, starts, K, frame, rot, masks, costs, dists, clears)
    assert (got["records"][..., 0] > 0).any() and (got["records"][..., 2] >= 0).all()


# ---------------------------------------------------------------- 3. rollout_arcs

def test_the_straight_arc_of_heading_zero_is_exact():
    rot = api.rotation_table(2.0 * np.pi * np.arange(16) / 16)
    arcs = api.rollout_arcs(rot, [1.0, 0.5, -0.25], [0.0], 12, unit=10)
    assert arcs.shape == (3, 12, 4) and arcs.dtype == np.int32
    t = np.arange(1, 13)
    assert np.array_equal(arcs[0], np.stack([16 * t, 0 * t, 0 * t, 10 + 0 * t], axis=1))
    assert np.array_equal(arcs[1], np.stack([8 * t, 0 * t, 0 * t, 5 + 0 * t], axis=1))
    assert np.array_equal(arcs[2], np.stack([-4 * t, 0 * t, 0 * t, 3 + 0 * t], axis=1))  # (floor(2.5 + 0.5) = 3)
    assert api.rollout_arcs(rot, [0.0], [0.0], 2, unit=10)[0].tolist() == [[0, 0, 0, 1], [0, 0, 0, 1]]  # (s is at least 1)


def test_arcs_keep_dk_in_range_and_left_mirrors_right():
    K = 16
    rot = api.rotation_table(2.0 * np.pi * np.arange(K) / K)
    turns = np.array([0.013, 0.05, 0.11, 0.27, 0.4])  # (none a multiple of half the heading spacing within 24 steps: no ties)
    arcs = api.rollout_arcs(rot, [0.3, 1.0, 2.5], np.concatenate([-turns, [0.0], turns]), 24)
    assert arcs.shape == (33, 24, 4)
    assert arcs[..., 2].min() >= 0 and arcs[..., 2].max() < K and (arcs[..., 3] >= 1).all()
    by = arcs.reshape(3, 11, 24, 4)
    for j in range(5):
        right, left = by[:, j], by[:, 6 + j]
        assert np.array_equal(left[..., 0], right[..., 0]) and np.array_equal(left[..., 1], -right[..., 1])
        assert np.array_equal(left[..., 2], (K - right[..., 2]) % K) and np.array_equal(left[..., 3], right[..., 3])
    # a quarter circle to the left at radius v / w: the pose is (r, r) and the heading a quarter of the table
    quarter = api.rollout_arcs(rot, [1.0], [math.pi / 32], 16)[0, 15]
    r = 16.0 / (math.pi / 32)
    assert abs(quarter[0] - r) <= 1 and abs(quarter[1] - r) <= 1 and quarter[2] == K // 4


def test_arcs_refuse():
    rot = api.rotation_table([0.0, 1.0])
    for bad in (dict(steps=0), dict(steps=129), dict(unit=0), dict(speeds=[]), dict(turns=[float("nan")]), dict(steps=2.0), dict(rotations=[[1, 2, 3]])):
        args = dict(rotations=rot, speeds=[1.0], turns=[0.0], steps=4)
        args.update(bad)
        with pytest.raises(ValueError):
            api.rollout_arcs(**args)


# ---------------------------------------------------------------- 4. the refusals of the Python method that need no device

def test_score_rollouts_refuses_before_the_device_is_looked_at():
    import torch

    seg = api.GroundSegmentation.__new__(api.GroundSegmentation)
    seg.rows = seg.cols = 20
    mask = torch.zeros((1, 20, 20), dtype=torch.int32)  # (a host tensor: the method refuses it, and everything before it first)
    table = torch.zeros((4, 2, 4), dtype=torch.int32)
    rot = api.rotation_table([0.0])
    for bad in (dict(order="diag"), dict(reach=-1), dict(reach=64), dict(reach=1.0), dict(cost_max=0), dict(cost_max=True), dict()):
        with pytest.raises(ValueError, match="score_rollouts"):
            seg.score_rollouts(mask, table, [(8, 8, 0)], rotations=rot, **bad)
