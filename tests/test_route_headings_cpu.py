"""gg_route_headings and gg_heading_moves without a GPU: the entry points are declared, exported, bound and reachable from C and Python, the
ctypes mirror has the layout the C compiler gives the struct, the ABI version is what it was, a null context is refused before the device
is touched.  gg_heading_moves (host arithmetic) is held word for word to tests/headings_ref.py.  And the expectation of the GPU tests
(headings_ref.expected_headings: a binary-heap Dijkstra over the reversed moves) is held without the code under test: against Bellman-Ford
sweeps over the whole volume and scipy's Dijkstra on the explicit graph, against closed forms, and on the two scenes the call exists for."""
import ctypes as C
import itertools
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
from tests import headings_ref as ref  # noqa: E402
from tests import route_ref  # noqa: E402

NONE = ref.NONE
INVALID = -1
SENTINEL = -77777
FIELDS = ["n", "d_mask", "mask_stride", "d_cost", "cost_stride", "d_goals", "goal_stride", "goal_headings", "n_headings", "moves", "cost_max", "max_cost",
          "order", "d_dist", "dist_stride", "plane_stride", "d_next", "next_stride", "next_plane_stride", "d_best", "best_stride", "d_best_heading",
          "best_heading_stride", "d_counts", "starts", "d_paths", "path_stride", "max_len", "d_path_len"]


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


def c_moves(lib, rotations, step, unit, turn, reverse_pct, spin, K=None):
    """gg_heading_moves as the C ABI has it: (status, table [K, 8, 4] prefilled with SENTINEL)"""
    rot = np.ascontiguousarray(np.asarray(rotations, np.int32).reshape(-1, 2))
    K = rot.shape[0] if K is None else K
    out = np.full((max(K, 1), 8, 4), SENTINEL, np.int32)
    rc = lib.gg_heading_moves(rot.ctypes.data_as(C.POINTER(C.c_int32)), K, step, unit, turn, reverse_pct, spin, out.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out


# ---------------------------------------------------------------- the ABI

def test_symbols_are_exported_and_bound(lib):
    for name, n_args in (("gg_route_headings", 3), ("gg_heading_moves", 8)):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == n_args


def test_struct_layout_equals_the_ctypes_mirror(lib):
    assert [f[0] for f in _lib.GGHeadingRoutes._fields_] == FIELDS
    lines = ['printf("%zu\\n", sizeof(gg_heading_routes));'] + [f'printf("%zu\\n", offsetof(gg_heading_routes, {k}));' for k in FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    assert [int(v) for v in out.split()] == [C.sizeof(_lib.GGHeadingRoutes)] + [getattr(_lib.GGHeadingRoutes, k).offset for k in FIELDS]


def test_feature_macro_and_the_limits_are_defined(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_ROUTE_HEADINGS) || GG_HAS_ROUTE_HEADINGS != 1
    #error "GG_HAS_ROUTE_HEADINGS"
    #endif
    int main(void) { printf("%d %d %d %d %d %d %d %d\n", GG_HAS_ROUTE_HEADINGS, GG_HEADINGS_MAX, GG_HEADINGS_MAX_MOVES, GG_HEADINGS_MAX_STEP,
                            GG_HEADINGS_MAX_COST, GG_HEADINGS_AT_GOAL, GG_ROUTE_NONE, GG_ABI_VERSION); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, 32, 8, 3, 32767, 8, NONE, 6]
    assert (_lib.GG_HAS_ROUTE_HEADINGS, _lib.GG_HEADINGS_MAX, _lib.GG_HEADINGS_MAX_MOVES, _lib.GG_HEADINGS_MAX_STEP, _lib.GG_HEADINGS_MAX_COST,
            _lib.GG_HEADINGS_AT_GOAL) == (1, ref.MAX_HEADINGS, ref.MAX_MOVES, ref.MAX_STEP, ref.MAX_COST, ref.AT_GOAL)
    assert _lib.GG_HEADINGS_LIMIT == ref.LIMIT == 2 ** 31 - 2
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION


def test_a_c_program_fills_the_struct_and_links(lib):
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int route(gg_context *ctx, const uint32_t *d_mask, const int32_t *d_frontier, const int32_t *moves, int32_t *d_dist, void *stream) {
        gg_heading_routes x = {0};
        x.n = 2;
        x.d_mask = d_mask;  x.mask_stride = 364 * 364;
        x.d_goals = d_frontier;  x.goal_stride = 364 * 364;
        x.goal_headings = 0xFFFFFFFFu;  x.n_headings = 16;  x.moves = moves;  x.cost_max = 1;  x.order = GG_PLANES_ROWMAJOR;
        x.d_dist = d_dist;  x.plane_stride = 364 * 364;  x.dist_stride = 16 * 364 * 364;
        return gg_route_headings(ctx, &x, stream);
    }
    int main(void) {
        const int32_t east[2] = {0, GG_MATCH_UNIT};
        int32_t moves[GG_HEADINGS_MAX_MOVES][4];
        if (gg_heading_moves(east, 1, 2, 10, 3, 150, 9, &moves[0][0]) != GG_OK) return 2;
        for (int m = 0; m < GG_HEADINGS_MAX_MOVES; ++m) printf("%d %d %d %d ", moves[m][0], moves[m][1], moves[m][2], moves[m][3]);
        printf("\n");
        return route(NULL, NULL, NULL, NULL, NULL, GG_STREAM_DEFAULT) == GG_ERR_INVALID ? 0 : 1;
    }
    ''')
    want = [[0, 2, 0, 20], [0, 2, 0, 23], [0, 2, 0, 23], [0, -2, 0, 30], [0, -2, 0, 35], [0, -2, 0, 35], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert [int(v) for v in out.split()] == [w for e in want for w in e]  # (K == 1: the turning moves keep the heading, no turn in place)


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGHeadingRoutes()
    x.n = 1
    assert lib.gg_route_headings(None, C.byref(x), None) == INVALID
    assert lib.gg_route_headings(None, None, None) == INVALID
    x.n = 0
    assert lib.gg_route_headings(None, C.byref(x), None) == INVALID


def test_the_mirrored_constants_are_the_kernels():
    internal = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    assert "inline int headings_tile(int n_headings) { return n_headings <= 16 ? 32 : 16; }" in internal
    assert [_lib.headings_tile(K) for K in (1, 16, 17, 32)] == [32, 32, 16, 16]
    for name, value in (("HEADINGS_MAX", 32), ("HEADINGS_MAX_MOVES", 8), ("HEADINGS_MAX_STEP", 3), ("HEADINGS_MAX_COST", 32767), ("HEADINGS_AT_GOAL", 8)):
        assert f"constexpr int {name} = {value};" in internal


# ---------------------------------------------------------------- gg_heading_moves

@pytest.mark.parametrize("K", [1, 2, 3, 4, 8, 16, 32])
def test_heading_moves_equal_the_restatement_word_for_word(lib, K):
    for offset, step, unit, turn, pct, spin in itertools.product((0.0, 0.3), (1, 2, 3), (1, 10, 1024), (0, 7), (0, 100, 175), (0, 11)):
        rot = ref.rotations(K, offset)
        rc, got = c_moves(lib, rot, step, unit, turn, pct, spin)
        want = ref.heading_moves(rot, step, unit, turn, pct, spin)
        assert want is not None and rc == 0 and got.tolist() == want, (K, offset, step, unit, turn, pct, spin)
        assert ref.moves_ok(got, K)
        assert np.array_equal(api.heading_moves(rot, step=step, unit=unit, turn=turn, reverse_pct=pct, spin=spin), got)
    assert np.array_equal(ref.rotations(K), api.rotation_table([2 * np.pi * k / K for k in range(K)]))


def test_heading_moves_by_hand(lib):
    # heading 1 of 8 looks along (cos 45, sin 45): one cell diagonally, floor(10 sqrt 2) = 14; three cells: (2, 2), floor(10 sqrt 8) = 28
    t = ref.table(8, 1, 10, turn=3, reverse_pct=150, spin=6)
    assert t[1].tolist() == [[1, 1, 1, 14], [1, 1, 2, 17], [1, 1, 0, 17], [-1, -1, 1, 21], [-1, -1, 2, 26], [-1, -1, 0, 26], [0, 0, 2, 6], [0, 0, 0, 6]]
    assert ref.table(8, 3, 10)[1, 0].tolist() == [2, 2, 1, 28]
    assert t[0, 2].tolist() == [1, 0, 7, 13] and t[7, 1].tolist() == [1, -1, 0, 17]  # the headings wrap
    # K = 2: both neighbours are the other heading
    t2 = ref.table(2, 1, 5, turn=1, spin=4)
    assert t2[0].tolist() == [[1, 0, 0, 5], [1, 0, 1, 6], [1, 0, 1, 6], [0] * 4, [0] * 4, [0] * 4, [0, 0, 1, 4], [0, 0, 1, 4]]
    # the zero pair: a heading whose axis rounds to (0, 0) keeps its turns in place alone; a short axis gives s = max(1, 0)
    rot = np.array([[0, 0], [8191, 0], [8192, 0], [-8192, 8191]], np.int32)
    rc, got = c_moves(lib, rot, 1, 1, 0, 100, 2)
    assert rc == 0 and got.tolist() == ref.heading_moves(rot, 1, 1, 0, 100, 2)
    assert got[0].tolist() == [[0] * 4] * 6 + [[0, 0, 1, 2], [0, 0, 3, 2]] and got[1, 0].tolist() == [0, 0, 0, 0]
    assert got[2, 0].tolist() == [1, 0, 2, 1] and got[3, 0].tolist() == [-1, 0, 3, 1] and got[3, 3].tolist() == [1, 0, 3, 1]


def test_heading_moves_refuse_with_the_table_untouched(lib):
    rot = ref.rotations(8)
    bad = [dict(step=0), dict(step=4), dict(unit=0), dict(unit=1025), dict(turn=-1), dict(spin=-1), dict(reverse_pct=99), dict(reverse_pct=-100),
           dict(reverse_pct=1), dict(spin=32768), dict(unit=1024, step=3, turn=29696), dict(unit=1024, step=3, reverse_pct=1100),
           dict(turn=2 ** 31 - 1), dict(reverse_pct=2 ** 31 - 1)]
    for kw in bad:
        p = dict(step=1, unit=10, turn=0, reverse_pct=0, spin=0)
        p.update(kw)
        rc, got = c_moves(lib, rot, p["step"], p["unit"], p["turn"], p["reverse_pct"], p["spin"])
        assert rc == INVALID and np.all(got == SENTINEL), kw
        assert ref.heading_moves(rot, **p) is None, kw
        with pytest.raises(ValueError):
            api.heading_moves(rot, **p)
    # the cost cap at its edge: 3 * 1024 = 3072 ahead, + 29695 = 32767 fits
    rc, got = c_moves(lib, rot, 3, 1024, 29695, 0, 0)
    assert rc == 0 and got[0, 1, 3] == 32767 and got.tolist() == ref.heading_moves(rot, 3, 1024, 29695, 0, 0)
    assert c_moves(lib, rot, 1, 10, 0, 0, 32767)[0] == 0
    for word in (16385, -16385):
        r2 = rot.copy()
        r2[5, 1] = word
        rc, got = c_moves(lib, r2, 1, 10, 0, 0, 0)
        assert rc == INVALID and np.all(got == SENTINEL) and ref.heading_moves(r2, 1, 10, 0, 0, 0) is None
    for K in (0, 33, -1):
        rc, got = c_moves(lib, ref.rotations(32), 1, 10, 0, 0, 0, K=K)
        assert rc == INVALID and np.all(got == SENTINEL)
    out = np.zeros((8, 8, 4), np.int32)
    assert lib.gg_heading_moves(None, 8, 1, 10, 0, 0, 0, out.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
    assert lib.gg_heading_moves(rot.ctypes.data_as(C.POINTER(C.c_int32)), 8, 1, 10, 0, 0, 0, None) == INVALID
    for bad_rot in (np.zeros((8, 3), np.int32), np.zeros((33, 2), np.int32), [[0.5, 0]]):
        with pytest.raises(ValueError):
            api.heading_moves(bad_rot)


# ---------------------------------------------------------------- the reference against two restatements that share no search with it

def bellman_ford(mask, goals, cost, moves, goal_headings, cost_max, reach=NONE - 1):
    """D by whole-volume sweeps of the recurrence to the fixed point; a tentative value above `reach` is not stored"""
    moves = np.asarray(moves)
    K = moves.shape[0]
    adm = ref.admissible_of(mask, K)
    w = ref.weights_of(cost, adm.shape[1:], cost_max)
    D = np.where(ref.goal_states(mask, goals, K, goal_headings), 0, NONE).astype(np.int64)
    for _ in range(D.size + 1):
        new = D.copy()
        for k in range(K):
            for da, db, k2, s in moves[k].tolist():
                if s:
                    cand = ref.shifted(D[k2], da, db, NONE) + s * ref.shifted(w, da, db, 0)
                    new[k] = np.where(adm[k] & (cand < new[k]) & (cand <= reach), cand, new[k])
        if np.array_equal(new, D):
            return D
        D = new
    raise AssertionError("no fixed point")


def hand_table(K):
    """a table no helper makes: an asymmetric 3-cell move, absent entries in the middle, a turn in place in one direction only"""
    t = np.zeros((K, 8, 4), np.int32)
    for k in range(K):
        t[k, 0] = (-3, 1, k, 31)
        t[k, 2] = (1, -2, (k + 1) % K, 17) if K > 1 else (1, -2, 0, 17)
        t[k, 5] = (0, 1, (k + K - 1) % K, 9)
        if K > 1:
            t[k, 7] = (0, 0, (k + 1) % K, 4)
    return t


def small_scenes():
    for (rows, cols), K in itertools.product(((9, 13), (20, 20)), (1, 4, 8)):
        rng = np.random.default_rng(rows * 100 + K)
        bits = (rng.random((K, rows, cols)) > 0.15) & (rng.random((rows, cols)) > 0.2)[None]
        mask = sum(bits[k].astype(np.int64) << k for k in range(K)) | (rng.integers(0, 2, (rows, cols)) << 31)
        mask = mask.astype(np.uint32).view(np.int32)
        cost = rng.integers(-3, 12, (rows, cols)).astype(np.int32)
        goals = np.where(rng.random((rows, cols)) < 0.03, 0, -1).astype(np.int32)
        tables = [ref.table(K, 1, 10, turn=2, reverse_pct=130, spin=5), ref.table(K, 2, 7, turn=1), hand_table(K)]
        for j, moves in enumerate(tables):
            yield f"{rows}x{cols} K={K} table {j}", mask, goals, cost, moves, (ref.ANY, 0b0101)[j % 2]


def test_reference_equals_bellman_ford_and_scipy():
    reached = 0
    for tag, mask, goals, cost, moves, gh in small_scenes():
        D = ref.cost_to_go(mask, goals, cost, moves, gh, 9)
        assert np.array_equal(D, bellman_ford(mask, goals, cost, moves, gh, 9)), tag
        assert np.array_equal(D, ref.graph_cost_to_go(mask, goals, cost, moves, gh, 9)), tag
        assert np.all(D[~ref.admissible_of(mask, moves.shape[0])] == NONE), tag
        reached += int(((D != NONE) & (D > 0)).sum())
    assert reached > 3000


def test_max_cost_acts_as_a_mask():
    for tag, mask, goals, cost, moves, gh in small_scenes():
        full = ref.expected_headings(mask, goals, cost, moves, gh, 9)
        finite = full["dist"][full["dist"] != NONE]
        if not len(finite):
            continue
        R = max(int(np.median(finite)), 1)
        cut = ref.expected_headings(mask, goals, cost, moves, gh, 9, max_cost=R)
        assert np.array_equal(cut["dist"], np.where(full["dist"] > R, NONE, full["dist"])), tag
        assert np.array_equal(cut["dist"], bellman_ford(mask, goals, cost, moves, gh, 9, reach=R)), tag  # (pruning while relaxing gives the same)
        keep = cut["dist"] != NONE
        assert np.array_equal(cut["next"][keep], full["next"][keep]) and np.all(cut["next"][~keep] == -1), tag
        assert cut["counts"].tolist() == [full["counts"][0], int(keep.sum()), full["counts"][2]], tag


# ---------------------------------------------------------------- closed forms

def four_moves(s):
    return np.array([[(-1, 0, 0, s), (0, -1, 0, s), (0, 1, 0, s), (1, 0, 0, s)] + [(0, 0, 0, 0)] * 4], np.int32)


def test_one_heading_and_four_unit_moves_equal_route_ref_at_connectivity_four():
    rng = np.random.default_rng(5)
    rows, cols = 17, 23
    blocked = np.where(rng.random((rows, cols)) < 0.3, 2, -1).astype(np.int32)
    cost = rng.integers(-3, 300, (rows, cols)).astype(np.int32)
    goals = np.where(rng.random((rows, cols)) < 0.02, 0, -1).astype(np.int32)
    mask = np.where(blocked < 0, 1, 0).astype(np.int32)
    for max_cost in (9000, 0):
        a = ref.expected_headings(mask, goals, cost, four_moves(5), cost_max=252, max_cost=max_cost)
        b = route_ref.expected_routes(goals, blocked, cost, route_ref.params(connectivity=4, straight=5, max_cost=max_cost))
        assert np.array_equal(a["dist"][0], b["dist"]) and np.array_equal(a["best"], b["dist"]) and a["counts"].tolist() == b["counts"].tolist()
        # the slots are route_ref's direction order: the same next cell
        rr, cc = np.mgrid[0:rows, 0:cols]
        step = np.array(route_ref.DIRECTIONS[:4] + ((0, 0),) * 5)  # (slot 8: a goal stays; -1 wraps to it and is masked below)
        cell = (rr + step[a["next"][0], 0]) * cols + cc + step[a["next"][0], 1]
        assert np.array_equal(np.where(a["next"][0] < 0, -1, cell), b["next"])
    assert int((b["dist"] != NONE).sum()) > 100  # (of the unbounded field, the last one computed)


def test_open_map_forward_only_closed_forms():
    """an open map of weight 1, K = 8, one goal cell: on the ray behind the goal along heading k the cost is n straight moves -- 10 n along an
    axis, 14 n along a diagonal, the Manhattan/diagonal form; no state is cheaper than that form of its offset; and with the goal heading
    fixed, the state one move away at the neighbouring heading pays the turn once"""
    side, K, turn = 21, 8, 3
    moves = ref.table(K, 1, 10, turn=turn)
    mask = np.full((side, side), (1 << K) - 1, np.int32)
    goals = np.full((side, side), -1, np.int32)
    g = side // 2
    goals[g, g] = 0
    D = ref.cost_to_go(mask, goals, None, moves)
    rr, cc = np.mgrid[0:side, 0:side]
    dr, dc = np.abs(rr - g), np.abs(cc - g)
    octile = 10 * np.abs(dr - dc) + 14 * np.minimum(dr, dc)
    assert np.all(D[:, g, g] == 0)
    for k in range(K):
        da, db, _, s = moves[k, 0].tolist()
        assert s == (10 if 0 in (da, db) else 14)
        for n in range(1, g + 1):
            assert D[k, g - n * da, g - n * db] == n * s == octile[g - n * da, g - n * db]
        assert np.all(D[k][D[k] != NONE] >= octile[D[k] != NONE])
    for k in range(K):  # the goal is heading k alone
        Dk = ref.cost_to_go(mask, goals, None, moves, 1 << k)
        for j in (-1, 1):
            k1 = (k + j) % K
            da, db, _, s = moves[k1, 0].tolist()
            assert Dk[k1, g - da, g - db] == s + turn  # one move that ends at heading k
            assert Dk[(k + 2 * j) % K, g - da - moves[(k + 2 * j) % K, 0, 0], g - db - moves[(k + 2 * j) % K, 0, 1]] == s + turn + moves[(k + 2 * j) % K, 0, 3] + turn
        assert Dk[k, g - moves[k, 0, 0], g - moves[k, 0, 1]] == moves[k, 0, 3]


def test_a_move_costs_the_cell_entered():
    mask = np.ones((1, 3), np.int32)
    goals = np.array([[-1, -1, 0]], np.int32)
    cost = np.array([[100, 7, 3]], np.int32)
    east = np.zeros((1, 8, 4), np.int32)
    east[0, 4] = (0, 1, 0, 2)
    e = ref.expected_headings(mask, goals, cost, east)
    assert e["dist"].tolist() == [[[2 * 7 + 2 * 3, 2 * 3, 0]]] and e["next"].tolist() == [[[4, 4, 8]]]
    jump = np.zeros((1, 8, 4), np.int32)
    jump[0, 1] = (0, 2, 0, 5)  # the cell between the two ends is not looked at
    assert ref.expected_headings(np.array([[1, 0, 1]], np.int32), goals, cost, jump)["dist"].tolist() == [[[15, NONE, 0]]]


def test_every_chain_of_next_falls_strictly_to_a_goal_state():
    mask, goals, cost, _, moves = ref.random_case(23, 8)
    e = ref.expected_headings(mask, goals, cost, moves)
    D, nxt = e["dist"].astype(np.int64), e["next"]
    w = ref.weights_of(cost, goals.shape, 252)
    walked = 0
    for k, r, c in np.argwhere((D != NONE) & (D > 0))[::7]:
        d = D[k, r, c]
        while d != 0:
            da, db, k2, s = moves[k, nxt[k, r, c]].tolist()
            assert s and D[k2, r + da, c + db] + s * w[r + da, c + db] == d
            k, r, c = k2, r + da, c + db
            assert D[k, r, c] < d
            d = D[k, r, c]
            walked += 1
        assert nxt[k, r, c] == ref.AT_GOAL
    assert walked > 1000


def test_tie_rules_the_smallest_slot_and_the_smallest_heading():
    moves = np.zeros((4, 8, 4), np.int32)
    for k in range(4):
        moves[k, 2] = (0, 1, k, 6)
        moves[k, 5] = (0, 1, k, 6)           # the same move again: slot 2 wins
        moves[k, 6] = (0, 1, (k + 1) % 4, 6)  # another heading at the same cost: slot 2 still wins
        moves[k, 1] = (0, 1, (k + 2) % 4, 7)  # a smaller slot that is dearer does not
    mask = np.array([[0b1111, 0b1110, 0b1111]], np.int32)
    goals = np.array([[-1, -1, 0]], np.int32)
    e = ref.expected_headings(mask, goals, None, moves)
    assert e["dist"][:, 0, :].tolist() == [[12, NONE, 0], [12, 6, 0], [12, 6, 0], [12, 6, 0]]
    assert e["next"][:, 0, :].tolist() == [[6, -1, 8], [2, 2, 8], [2, 2, 8], [2, 2, 8]]  # (heading 0 is not admissible in the middle: slot 6 leads round it)
    assert e["best"].tolist() == [[12, 6, 0]] and e["best_heading"].tolist() == [[0, 1, 0]]
    assert e["counts"].tolist() == [4, 11, 11]
    none = ref.expected_headings(mask, goals, None, moves, goal_headings=0xFFFFFFF0)
    assert np.all(none["dist"] == NONE) and np.all(none["best_heading"] == -1) and none["counts"].tolist() == [0, 0, 11]


def test_the_overflow_limit_at_its_edge():
    moves = four_moves(32767)
    rows = cols = 16
    cost_max = ref.LIMIT // (32767 * rows * cols)
    assert ref.within_limit(rows, cols, 1, moves, cost_max) and not ref.within_limit(rows, cols, 1, moves, cost_max + 1)
    assert 32767 * cost_max * rows * cols <= 2 ** 31 - 2 < 32767 * (cost_max + 1) * rows * cols
    # at the limit the dearest chain still fits: a serpentine through every cell of a 16 x 16 map at cost_max
    mask = np.ones((rows, cols), np.int32)
    for r in range(1, rows, 2):
        mask[r, :] = 0
        mask[r, cols - 1 if (r // 2) % 2 == 0 else 0] = 1
    goals = np.full((rows, cols), -1, np.int32)
    goals[0, 0] = 0
    D = ref.cost_to_go(mask, goals, np.full((rows, cols), 2 ** 31 - 1, np.int32), moves, cost_max=cost_max)
    assert NONE > D[D != NONE].max() == 32767 * cost_max * (int(mask.sum()) - 1) > 2 ** 30


# ---------------------------------------------------------------- the two scenes the call exists for

@pytest.mark.parametrize("name", ["dead_end", "l_bend"])
def test_purpose_scenes(name):
    side = 20
    mask, goals, cost, start, gh = ref.dead_end(side) if name == "dead_end" else ref.l_bend(side)
    K = 8 if name == "dead_end" else 4
    r0, c0, k0 = start
    # the projection "fits at some heading" lets gg_route_planes through
    proj = np.where(ref.admissible_of(mask, K).any(axis=0), -1, 0).astype(np.int32)
    flat = route_ref.expected_routes(goals, proj, None, route_ref.params(connectivity=4))
    assert flat["dist"][r0, c0] != NONE
    st = (ref.linear(r0, c0, side, side, "row"), k0)
    forward = ref.expected_headings(mask, goals, cost, ref.table(K, 1, 10, turn=2), gh, start=st, max_len=64)
    assert forward["dist"][k0, r0, c0] == NONE and forward["path_len"] == 0 and forward["counts"][0] >= 1
    both = ref.expected_headings(mask, goals, cost, ref.table(K, 1, 10, turn=2, reverse_pct=150), gh, start=st, max_len=64)
    assert both["dist"][k0, r0, c0] != NONE and 2 <= both["path_len"] <= 64
    slots = [int(both["next"][k][ref.cell_of(cell, side, side, "row")]) for cell, k in both["whole_path"]]
    assert slots[-1] == ref.AT_GOAL and any(3 <= m <= 5 for m in slots), slots
    last_cell, last_k = both["whole_path"][-1]
    assert goals[ref.cell_of(last_cell, side, side, "row")] >= 0 and (gh >> last_k) & 1


# ---------------------------------------------------------------- the scene classes of the GPU tests' random scenes

@pytest.mark.parametrize("side", ref.RANDOM_SIDES)
def test_random_scenes_of_the_gpu_tests_hold_every_class(side):
    steps, reverse, spin = set(), set(), set()
    for K in ref.RANDOM_HEADINGS:
        mask, goals, cost, _, moves = ref.random_case(side, K)
        want = ref.expected_headings(mask, goals, cost, moves)
        n_goal, n_turning, n_unreached = ref.scene_classes(want, moves)
        assert n_goal >= 10 and n_turning >= 100 and n_unreached >= 10, (side, K, n_goal, n_turning, n_unreached)
        assert (np.asarray(mask).view(np.uint32) >> K).any() or K == 32  # mask bits above K are set
    for s, K in itertools.product(ref.RANDOM_SIDES, ref.RANDOM_HEADINGS):
        t = ref.random_table(s, K)
        steps.add(int(np.abs(t[0, 0, :2]).max()))
        reverse.add(bool(t[:, 3, 3].any()))
        spin.add(bool(t[:, 6, 3].any()))
    assert steps == {1, 2, 3} and reverse == {False, True} and spin == {False, True}
