"""gg_route_planes without a GPU: the entry point is declared, exported, bound and reachable from C and Python, the ctypes mirror has the
layout the C compiler gives the struct, the ABI version is what it was, a null context is refused before the device is touched, and the
Python entry point refuses bad arguments before any library call.  And the expectation of the GPU tests (tests/route_ref.py, a binary-heap
Dijkstra) is held without the code under test: against whole-map Bellman-Ford sweeps to the fixed point, against scipy's Dijkstra on the
explicitly built directed graph, and on closed forms and facts fixed by hand."""
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
from tests import route_ref  # noqa: E402

NONE = route_ref.NONE
FIELDS = ["n", "d_blocked", "blocked_stride", "d_cost", "cost_stride", "d_goals", "goal_stride", "connectivity", "straight", "diagonal", "cost_max",
          "max_cost", "order", "d_dist", "plane_stride", "d_next", "d_counts", "starts", "d_paths", "max_path", "d_path_len"]


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
    assert "gg_route_planes" in _lib.SYMBOLS
    assert hasattr(lib, "gg_route_planes")
    assert len(lib.gg_route_planes.argtypes) == 3


def test_struct_layout_equals_the_ctypes_mirror(lib):
    assert [f[0] for f in _lib.GGPlaneRoutes._fields_] == FIELDS
    lines = ['printf("%zu\\n", sizeof(gg_plane_routes));'] + [f'printf("%zu\\n", offsetof(gg_plane_routes, {k}));' for k in FIELDS]
    out = compile_and_run(r'''
    #include <stddef.h>
    #include <stdio.h>
    #include "groundgrid_hip.h"
    int main(void) { ''' + " ".join(lines) + " return 0; }")
    assert [int(v) for v in out.split()] == [C.sizeof(_lib.GGPlaneRoutes)] + [getattr(_lib.GGPlaneRoutes, k).offset for k in FIELDS]


def test_feature_macro_and_the_unreached_word_are_defined(lib):
    out = compile_and_run(r'''
    #include <stdio.h>
    #include "groundgrid_hip.h"
    #if !defined(GG_HAS_ROUTE_PLANES) || GG_HAS_ROUTE_PLANES != 1
    #error "GG_HAS_ROUTE_PLANES"
    #endif
    int main(void) { printf("%d %d %d\n", GG_HAS_ROUTE_PLANES, GG_ROUTE_NONE, GG_ABI_VERSION); return 0; }
    ''')
    assert [int(v) for v in out.split()] == [1, NONE, 6]
    assert _lib.GG_HAS_ROUTE_PLANES == 1 and _lib.GG_ROUTE_NONE == NONE == 2 ** 31 - 1
    assert lib.gg_abi_version() == 6 == _lib.GG_ABI_VERSION


def test_a_c_program_fills_the_struct_and_links(lib):
    compile_and_run(r'''
    #include <stddef.h>
    #include "groundgrid_hip.h"
    int route(gg_context *ctx, const int32_t *d_fused, const int32_t *d_cost, const int32_t *d_frontier, int32_t *d_dist, int32_t *d_next, int32_t *d_counts,
              const int32_t *starts, int32_t *d_paths, int32_t *d_path_len, void *stream) {
        gg_plane_routes x = {0};
        x.n = 2;
        x.d_blocked = d_fused;  x.blocked_stride = 364 * 364;
        x.d_cost = d_cost;  x.cost_stride = 364 * 364;
        x.d_goals = d_frontier;  x.goal_stride = 364 * 364;
        x.connectivity = 8;  x.straight = 5;  x.diagonal = 7;  x.cost_max = 252;  x.max_cost = 0;
        x.order = GG_PLANES_ROWMAJOR;
        x.d_dist = d_dist;  x.plane_stride = 364 * 364;
        x.d_next = d_next;
        x.d_counts = d_counts;
        x.starts = starts;  x.d_paths = d_paths;  x.max_path = 1024;  x.d_path_len = d_path_len;
        return gg_route_planes(ctx, &x, stream);
    }
    int main(void) { return route(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, GG_STREAM_DEFAULT) == GG_ERR_INVALID ? 0 : 1; }
    ''')


def test_null_context_and_null_struct_are_invalid(lib):
    x = _lib.GGPlaneRoutes()
    x.n = 1
    assert lib.gg_route_planes(None, C.byref(x), None) == -1  # GG_ERR_INVALID
    assert lib.gg_route_planes(None, None, None) == -1
    x.n = 0
    assert lib.gg_route_planes(None, C.byref(x), None) == -1


def test_the_mirrored_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "groundgrid_amd", "csrc", "gg_internal.h")).read()
    assert int(re.search(r"constexpr int ROUTE_TILE = (\d+);", text).group(1)) == _lib.GG_ROUTE_TILE
    assert _lib.GG_ROUTE_LIMIT == route_ref.LIMIT == 2 ** 31 - 2


# ---------------------------------------------------------------- the Python entry point

def test_python_entry_point_exists():
    params = inspect.signature(api.GroundSegmentation.route_planes).parameters
    assert list(params)[:4] == ["self", "goals", "blocked", "cost"]
    assert params["blocked"].default is None and params["cost"].default is None
    defaults = {**route_ref.DEFAULTS, "order": "row", "next": True, "counts": True, "starts": None, "max_path": 0, "out": None, "on_torch_stream": False}
    assert list(params)[4:] == list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[name].default is default or params[name].default == default, name
    assert [f for f in api.RouteOutputs.__dataclass_fields__] == ["dist", "next", "counts", "paths", "path_len"]


class NoLibrary:
    """in place of the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


def test_python_entry_point_refuses_bad_arguments_before_any_library_call(lib):
    import torch

    seg = api.GroundSegmentation()
    seg._L, seg.rows, seg.cols, seg.device, seg.n_slots = NoLibrary(), 20, 20, 0, 4
    host = torch.zeros((2, 20, 20), dtype=torch.int32)
    with pytest.raises(ValueError):  # (not on the device)
        seg.route_planes(host)
    for bad in (None, np.zeros((2, 20, 20), np.int32), "planes"):
        with pytest.raises(ValueError):
            seg.route_planes(bad)
    for kw in (dict(order="fortran"), dict(connectivity=6), dict(connectivity=True), dict(straight=0), dict(straight=65536), dict(diagonal=0), dict(diagonal=65536),
               dict(straight=1.5), dict(cost_max=0), dict(max_cost=-1), dict(cost_max=None), dict(straight=65535, cost_max=82),
               dict(connectivity=4, straight=5, cost_max=1073742), dict(max_path=-1)):
        with pytest.raises(ValueError, match=r"route_planes: (?!goals must)"):  # (the parameter is named, not the planes)
            seg.route_planes(host, **kw)


def test_goal_planes_puts_the_cells_where_the_order_says():
    got = api.goal_planes([[(1, 2), (0, 0)], [], [(2, 3)]], 3, 4)
    assert tuple(got.shape) == (3, 3, 4) and got.dtype.is_signed and not got.is_cuda
    want = np.full((3, 3, 4), -1, np.int32)
    want[0, 1, 2] = want[0, 0, 0] = want[2, 2, 3] = 0
    assert np.array_equal(got.numpy(), want)
    col = api.goal_planes([[(1, 2)]], 3, 4, order="col")
    one = np.full((3, 4), -1, np.int32)
    one[1, 2] = 0
    assert tuple(col.shape) == (1, 4, 3) and np.array_equal(col.numpy()[0], route_ref.lay(one, "col"))
    with pytest.raises(ValueError):
        api.goal_planes([[(3, 0)]], 3, 4)


# ---------------------------------------------------------------- the reference, without the code under test

def bellman_ford(goals, blocked, cost, p):
    """a second restatement that shares no search with route_ref: whole-map sweeps of D(q) = min(D(q), D(p) + s * w(p)) over shifted copies
    of the planes, until a sweep changes nothing"""
    goals = np.asarray(goals)
    rows, cols = goals.shape
    B = np.zeros(goals.shape, bool) if blocked is None else np.asarray(blocked) >= 0
    w = np.ones(goals.shape, np.int64) if cost is None else np.clip(np.asarray(cost).astype(np.int64), 1, p["cost_max"])
    INF = 1 << 60
    D = np.where((goals >= 0) & ~B, 0, INF).astype(np.int64)

    def shifted(a, da, db, fill):
        """out[r, c] = a[r + da, c + db] where that cell exists, `fill` elsewhere"""
        out = np.full(a.shape, fill, a.dtype)
        rs, re_ = max(0, -da), min(rows, rows - da)
        cs, ce = max(0, -db), min(cols, cols - db)
        out[rs:re_, cs:ce] = a[rs + da:re_ + da, cs + db:ce + db]
        return out

    for _ in range(rows * cols + 1):
        new = D.copy()
        for k, (a, b) in enumerate(route_ref.DIRECTIONS[:p["connectivity"]]):
            s = p["straight"] if k < 4 else p["diagonal"]
            ok = ~B & ~shifted(B, a, b, True)
            if k >= 4:
                ok &= ~shifted(B, a, 0, True) & ~shifted(B, 0, b, True)
            cand = shifted(D, a, b, INF) + s * shifted(w, a, b, 0)
            new = np.where(ok & (cand < new), cand, new)
        if np.array_equal(new, D):
            break
        D = new
    else:
        raise AssertionError("no fixed point")
    return np.where(D >= INF, NONE, D)


def scipy_dijkstra(goals, blocked, cost, p):
    """a third: scipy.sparse.csgraph.dijkstra on the explicitly built directed graph, edge p -> q of weight s * w(p) for every admissible
    step q -> p (the search runs from the goals against the steps)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    goals = np.asarray(goals)
    rows, cols = goals.shape
    B = np.zeros(goals.shape, bool) if blocked is None else np.asarray(blocked) >= 0
    w = np.ones(goals.shape, np.int64) if cost is None else np.clip(np.asarray(cost).astype(np.int64), 1, p["cost_max"])
    src, dst, wt = [], [], []
    for r in range(rows):
        for c in range(cols):
            if B[r, c]:
                continue
            for k, (a, b) in enumerate(route_ref.DIRECTIONS[:p["connectivity"]]):
                pr, pc = r + a, c + b
                if not (0 <= pr < rows and 0 <= pc < cols) or B[pr, pc]:
                    continue
                if k >= 4 and (B[r + a, c] or B[r, c + b]):
                    continue
                src.append(pr * cols + pc)  # the step (r, c) -> (pr, pc) enters (pr, pc)
                dst.append(r * cols + c)
                wt.append((p["straight"] if k < 4 else p["diagonal"]) * int(w[pr, pc]))
    G = csr_matrix((np.array(wt, np.float64), (np.array(src, np.int64), np.array(dst, np.int64))), shape=(rows * cols, rows * cols))
    sources = np.flatnonzero(((goals >= 0) & ~B).ravel())
    if len(sources) == 0:
        return np.full(goals.shape, NONE, np.int64)
    d = dijkstra(G, directed=True, indices=sources, min_only=True)  # (every sum is an integer far below 2^53: exact in float64)
    return np.where(np.isinf(d), NONE, d).astype(np.int64).reshape(rows, cols)


def random_map(rng, rows, cols, n_goals, with_cost, density=0.3):
    blocked = np.where(rng.random((rows, cols)) < density, rng.integers(0, 3, (rows, cols)), -1).astype(np.int32)
    cost = rng.integers(-3, 300, (rows, cols)).astype(np.int32) if with_cost else None  # (words <= 0 and > cost_max: clamped)
    goals = np.full((rows, cols), -1, np.int32)
    for _ in range(n_goals):
        goals[rng.integers(rows), rng.integers(cols)] = rng.integers(0, 5)
    return goals, blocked, cost


CASES = [(shape, conn, with_cost, n_goals) for shape in ((9, 13), (20, 20)) for conn in (4, 8) for with_cost in (False, True) for n_goals in (0, 1, 4)]


@pytest.mark.parametrize("shape,conn,with_cost,n_goals", CASES)
def test_reference_equals_bellman_ford_and_scipy(shape, conn, with_cost, n_goals):
    rng = np.random.default_rng(1900 + 97 * shape[0] + 11 * conn + 3 * n_goals + with_cost)
    p = route_ref.params(connectivity=conn)
    for _ in range(3):
        goals, blocked, cost = random_map(rng, *shape, n_goals, with_cost)
        D = route_ref.cost_to_go(goals, blocked, cost, p)
        assert np.array_equal(D, bellman_ford(goals, blocked, cost, p))
        assert np.array_equal(D, scipy_dijkstra(goals, blocked, cost, p))
        if n_goals == 0:
            assert (D == NONE).all()


def test_open_map_closed_forms():
    rows, cols = 11, 14
    goals = np.full((rows, cols), -1, np.int32)
    goals[4, 9] = 0
    dr, dc = np.abs(np.arange(rows)[:, None] - 4), np.abs(np.arange(cols)[None, :] - 9)
    four = route_ref.expected_routes(goals, p=route_ref.params(connectivity=4, straight=3))
    assert np.array_equal(four["dist"], 3 * (dr + dc))
    eight = route_ref.expected_routes(goals, p=route_ref.params())
    assert np.array_equal(eight["dist"], 7 * np.minimum(dr, dc) + 5 * np.abs(dr - dc))
    assert four["counts"].tolist() == eight["counts"].tolist() == [1, rows * cols, rows * cols]


def test_a_diagonal_gap_is_not_passed_and_a_blocked_goal_is_no_goal():
    blocked = np.full((4, 4), -1, np.int32)
    blocked[0, 1] = blocked[1, 0] = 0  # (0, 0) touches the rest of the map through the diagonal gap alone
    goals = np.full((4, 4), -1, np.int32)
    goals[3, 3] = 0
    got = route_ref.expected_routes(goals, blocked)
    assert got["dist"][0, 0] == NONE and got["next"][0, 0] == -1 and got["dist"][1, 1] == 14
    assert got["counts"].tolist() == [1, 13, 14]
    blocked[1, 0] = -1  # one side cell free is not enough for the diagonal; the straight way round is open now
    assert route_ref.expected_routes(goals, blocked)["dist"][0, 0] == 14 + 5 + 5
    goals[0, 1] = 0  # a goal on a blocked cell
    got = route_ref.expected_routes(goals, blocked)
    assert got["counts"][0] == 1 and got["dist"][0, 1] == NONE and got["dist"][0, 0] == 24


def test_the_cost_of_a_step_is_that_of_the_cell_entered():
    cost = np.array([[1, 10, 100, 1000]], np.int32)
    goals = np.array([[-1, -1, -1, 0]], np.int32)
    got = route_ref.expected_routes(goals, None, cost, route_ref.params(connectivity=4, straight=2, cost_max=500))
    assert got["dist"].tolist() == [[2 * (10 + 100 + 500), 2 * (100 + 500), 2 * 500, 0]]  # (1000 is clamped; the start's own cost never counts)


@pytest.mark.parametrize("order", ["row", "col"])
@pytest.mark.parametrize("conn", [4, 8])
def test_every_next_chain_falls_strictly_and_ends_on_a_goal(conn, order):
    rng = np.random.default_rng(1950 + conn)
    rows, cols = 17, 12
    goals, blocked, cost = random_map(rng, rows, cols, 3, True, density=0.25)
    got = route_ref.expected_routes(goals, blocked, cost, route_ref.params(connectivity=conn), order)
    D, nxt = got["dist"], got["next"]
    assert (D != NONE).sum() > rows * cols // 3
    for r in range(rows):
        for c in range(cols):
            if D[r, c] == NONE:
                assert nxt[r, c] == -1
                continue
            here, steps = (r, c), 0
            while D[here] != 0:
                there = route_ref.cell_of(int(nxt[here]), rows, cols, order)
                assert max(abs(there[0] - here[0]), abs(there[1] - here[1])) == 1 and D[there] <= D[here] - 1
                here, steps = there, steps + 1
                assert steps <= rows * cols
            assert goals[here] >= 0 and blocked[here] < 0 and nxt[here] == route_ref.linear(*here, rows, cols, order)


def test_ties_take_the_first_direction_of_the_order():
    goals = np.full((7, 7), -1, np.int32)
    goals[3, 3] = 0
    got = route_ref.expected_routes(goals, p=route_ref.params(straight=1, diagonal=1))  # every neighbour nearer the goal attains the minimum
    want = {(0, 0): (1, 1), (0, 3): (1, 3), (0, 6): (1, 5), (3, 0): (3, 1), (3, 6): (3, 5), (6, 0): (5, 1), (6, 3): (5, 3), (6, 6): (5, 5),
            (0, 1): (1, 1), (0, 2): (1, 2), (1, 0): (1, 1), (2, 0): (2, 1), (6, 1): (5, 1), (6, 2): (5, 2), (1, 6): (1, 5), (0, 5): (1, 5), (0, 4): (1, 4)}
    for q, p_ in want.items():
        assert route_ref.cell_of(int(got["next"][q]), 7, 7, "row") == p_, q


def test_paths_and_their_truncation():
    goals = np.full((1, 6), -1, np.int32)
    goals[0, 5] = 0
    blocked = np.full((1, 6), -1, np.int32)
    got = route_ref.expected_routes(goals, blocked, start=1, max_path=8, sentinel=-7)
    assert got["path_len"] == 5 and got["path"].tolist() == [1, 2, 3, 4, 5, -7, -7, -7]
    cut = route_ref.expected_routes(goals, blocked, start=1, max_path=3, sentinel=-7)
    assert cut["path_len"] == 5 and cut["path"].tolist() == [1, 2, 3]
    on_goal = route_ref.expected_routes(goals, blocked, start=5, max_path=2, sentinel=-7)
    assert on_goal["path_len"] == 1 and on_goal["path"].tolist() == [5, -7]
    blocked[0, 3] = 0
    for start in (-1, 1, 3):  # no start, a pocket, a blocked cell
        none = route_ref.expected_routes(goals, blocked, start=start, max_path=2, sentinel=-7)
        assert none["path_len"] == 0 and none["path"].tolist() == [-7, -7]
    beyond = route_ref.expected_routes(goals, None, p=route_ref.params(max_cost=10), start=2, max_path=2, sentinel=-7)
    assert beyond["path_len"] == 0 and beyond["dist"].tolist() == [[NONE, NONE, NONE, 10, 5, 0]]
    col = route_ref.expected_routes(goals.T, None, order="col", start=1, max_path=8, sentinel=-7)  # a 6 x 1 map: the same plane column-major
    assert col["path"].tolist() == got["path"].tolist()


def test_max_cost_equals_masking_the_unbounded_result():
    rng = np.random.default_rng(1977)
    goals, blocked, cost = random_map(rng, 20, 20, 2, True, density=0.2)
    free = route_ref.expected_routes(goals, blocked, cost)
    reached = np.sort(free["dist"][free["dist"] != NONE])
    R = int(reached[len(reached) // 2])
    got = route_ref.expected_routes(goals, blocked, cost, route_ref.params(max_cost=R))
    keep = free["dist"] <= R
    assert 0 < keep.sum() < (free["dist"] != NONE).sum()
    assert np.array_equal(got["dist"], np.where(keep, free["dist"], NONE)) and np.array_equal(got["next"], np.where(keep, free["next"], -1))
    assert got["counts"].tolist() == [free["counts"][0], int(keep.sum()), free["counts"][2]]


def test_the_overflow_limit_at_its_edge():
    # max(straight, diagonal) * cost_max * rows * cols <= 2^31 - 2, the diagonal counted with connectivity 8 only
    assert route_ref.within_limit(364, 364, route_ref.params())  # 7 * 252 * 132496
    cells = 20 * 20
    top = (2 ** 31 - 2) // (7 * cells)
    assert route_ref.within_limit(20, 20, route_ref.params(cost_max=top)) and not route_ref.within_limit(20, 20, route_ref.params(cost_max=top + 1))
    top4 = (2 ** 31 - 2) // (5 * cells)
    assert top4 > top
    assert route_ref.within_limit(20, 20, route_ref.params(connectivity=4, cost_max=top4, diagonal=10 ** 9))
    assert not route_ref.within_limit(20, 20, route_ref.params(connectivity=4, cost_max=top4 + 1))
    assert not route_ref.within_limit(20, 20, route_ref.params(cost_max=top4))
    assert route_ref.within_limit(1, 1, route_ref.params(straight=1, diagonal=1, cost_max=2 ** 31 - 2))
    assert not route_ref.within_limit(1, 1, route_ref.params(straight=1, diagonal=1, cost_max=2 ** 31 - 1))
    for bad in (dict(straight=0), dict(straight=65536), dict(diagonal=0), dict(diagonal=65536), dict(cost_max=0)):
        assert not route_ref.within_limit(2, 2, route_ref.params(**bad))
    # at the edge the longest conceivable path still fits: every cell entered once at the largest step
    assert 7 * top * (cells - 1) < NONE
