"""gg_route_planes (the cost-to-go, next-cell and path outputs of many maps over caller-given goal, blocked and cost planes, in device memory)
on the device.  Expected values come from numpy alone (tests/route_ref.py: a binary-heap Dijkstra, held against Bellman-Ford sweeps and
scipy's Dijkstra by tests/test_route_planes_cpu.py).  Every comparison is on bits: every cell of d_dist and d_next, the counts, the path
rows and lengths, the words between rows * cols and the stride and behind the last plane."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402
from tests import route_ref  # noqa: E402
from tests.test_export_layers_gpu import POSE, batch_points, fresh_count, same_bits, stride_of  # noqa: E402
from tests.test_fuse_states_gpu import GEOMETRY, MAX_POINTS, SIGNED_SENTINEL, pack, scan_cloud  # noqa: E402
from tests.test_split_clouds_gpu import PARAM_RING, lazy_count  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
NONE = route_ref.NONE
TILE = _lib.GG_ROUTE_TILE
PLANES = ("dist", "next")
ROWS = ("counts", "paths", "path_len")


# ---------------------------------------------------------------- helpers

@pytest.fixture(scope="module")
def contexts():
    """one context per (side, slots), made on demand and shared: no call of this file but the drive's changes a map"""
    made = {}

    def get(side, n_slots=5):
        if (side, n_slots) not in made:
            length, res = GEOMETRY[side] if side in GEOMETRY else (120.0, 0.33)
            seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=MAX_POINTS)
            assert seg.rows == seg.cols == side
            made[(side, n_slots)] = seg
        return made[(side, n_slots)]

    yield get
    for seg in made.values():
        seg.close()


class Dest:
    """sentinel-filled destinations of one call: n planes of dist and next plane_stride words apart (and `slack` words behind), the counts,
    the path rows of max_path words and the path lengths, each with a few words behind"""

    def __init__(self, n, plane_stride, max_path=1, slack=0):
        import torch

        self.n, self.plane_stride, self.max_path = n, plane_stride, max_path
        for k in PLANES:
            setattr(self, k, torch.full((max(n * plane_stride + slack, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda"))
        self.counts = torch.full((3 * max(n, 1) + 3,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.paths = torch.full((max(n, 1) * max_path + 5,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.path_len = torch.full((max(n, 1) + 3,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in PLANES + ROWS}

    def all_sentinel(self):
        return all(bool((getattr(self, k) == SIGNED_SENTINEL).all().item()) for k in PLANES + ROWS)


def raw_route(seg, n, dest, goals, goal_stride, blocked=None, blocked_stride=0, cost=None, cost_stride=0, p=None, order=ROW, give=("next", "counts"),
              starts=None, stream=None, own=False, **over):
    """gg_route_planes as the C ABI has it (goals, blocked, cost: device tensors or addresses, 0 / None = null; starts: [n] or None); returns
    the status.  `give`: the nullable outputs handed over; `over`: dist, next, counts, paths, path_len, plane_stride, max_path in place of
    `dest`'s"""
    import torch

    def address(t):
        return (t.data_ptr() if torch.is_tensor(t) else t) or None

    p = p or route_ref.params()
    x = _lib.GGPlaneRoutes()
    x.n, x.d_goals, x.goal_stride = n, address(goals), goal_stride
    x.d_blocked, x.blocked_stride, x.d_cost, x.cost_stride = address(blocked), blocked_stride, address(cost), cost_stride
    x.connectivity, x.straight, x.diagonal, x.cost_max, x.max_cost, x.order = p["connectivity"], p["straight"], p["diagonal"], p["cost_max"], p["max_cost"], order
    x.d_dist, x.plane_stride = address(over.get("dist", dest.dist)), over.get("plane_stride", dest.plane_stride)
    x.d_next = address(over.get("next", dest.next if "next" in give else 0))
    x.d_counts = address(over.get("counts", dest.counts if "counts" in give else 0))
    st = None
    if starts is not None:
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1))
        x.starts = st.ctypes.data_as(C.POINTER(C.c_int32))
    x.d_paths, x.max_path, x.d_path_len = address(over.get("paths", dest.paths)), over.get("max_path", dest.max_path), address(over.get("path_len", dest.path_len))
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_route_planes(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check_map(host, i, want, order, dest, tag, give=("next", "counts"), with_paths=True):
    """map i of a downloaded Dest against route_ref.expected_routes: every cell of every given plane, the counts, the path row and length, the
    words behind every plane, and the outputs that were not handed over"""
    cells, stride = want["dist"].size, dest.plane_stride
    for k in PLANES:
        words = host[k][i * stride: (i + 1) * stride]
        if k == "next" and "next" not in give:
            assert np.all(words == SIGNED_SENTINEL), f"{tag}: map {i}: next was not handed over and was written"
            continue
        laid = route_ref.lay(want[k], ORDER[order])
        got = words[:cells].reshape(laid.shape)
        bad = np.argwhere(got != laid)
        assert len(bad) == 0, f"{tag}: map {i}: {k}: {len(bad)} cells differ, first {tuple(bad[0])}: {got[tuple(bad[0])]} != {laid[tuple(bad[0])]}"
        assert np.all(words[cells:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words behind the {k} plane were written"
    counts = host["counts"][3 * i: 3 * i + 3]
    if "counts" in give:
        assert counts.tolist() == want["counts"].tolist(), f"{tag}: map {i}: counts {counts} != {want['counts']}"
    else:
        assert np.all(counts == SIGNED_SENTINEL), f"{tag}: map {i}: the counts were not handed over and were written"
    row, length = host["paths"][i * dest.max_path: (i + 1) * dest.max_path], host["path_len"][i]
    if with_paths:
        assert length == want["path_len"], f"{tag}: map {i}: path_len {length} != {want['path_len']}"
        assert np.array_equal(row, want["path"]), f"{tag}: map {i}: the path row differs"
    else:
        assert length == SIGNED_SENTINEL and np.all(row == SIGNED_SENTINEL), f"{tag}: map {i}: no starts were given and the paths were written"


def check_tail(host, dest, tag):
    n = dest.n
    for k in PLANES:
        assert np.all(host[k][n * dest.plane_stride:] == SIGNED_SENTINEL), f"{tag}: the words behind the last {k} plane were written"
    assert np.all(host["counts"][3 * n:] == SIGNED_SENTINEL) and np.all(host["paths"][n * dest.max_path:] == SIGNED_SENTINEL)
    assert np.all(host["path_len"][n:] == SIGNED_SENTINEL), f"{tag}: the words behind the counts, paths or lengths were written"


# ---------------------------------------------------------------- scenes: (goals, blocked, cost, start cell) as logical [side, side] planes

def open_map(side):
    return np.full((side, side), -1, np.int32)


def random_field(side, seed, density=0.3, n_goals=1):
    """30 % blocked (several non-negative words), costs across and beyond [1, cost_max], goals anywhere (some on blocked cells)"""
    rng = np.random.default_rng(seed)
    blocked = np.where(rng.random((side, side)) < density, rng.integers(0, 3, (side, side)), rng.integers(-3, 0, (side, side))).astype(np.int32)
    cost = rng.integers(-5, 300, (side, side)).astype(np.int32)
    cost[rng.random((side, side)) < 0.02] = -2 ** 31
    cost[rng.random((side, side)) < 0.02] = 2 ** 31 - 1
    goals = open_map(side)
    for _ in range(n_goals):
        goals[rng.integers(side), rng.integers(side)] = rng.integers(0, 9)
    free = np.argwhere(blocked < 0)
    goals[tuple(free[len(free) // 2])] = 0  # (at least one goal that is none on a blocked cell)
    return goals, blocked, cost, tuple(free[-1])


def serpentine(side):
    """corridors one cell wide along the even rows, joined at alternating ends: the path from the last corridor to the goal at (0, 0) walks
    every one of them, leaving and re-entering the same tiles"""
    blocked = open_map(side)
    for r in range(1, side, 2):
        blocked[r, :] = 0
        blocked[r, side - 1 if (r // 2) % 2 == 0 else 0] = -1
    goals = open_map(side)
    goals[0, 0] = 0
    last = (side - 1) // 2 * 2
    return goals, blocked, None, (last, side - 1 if (last // 2) % 2 == 0 else 0)


def detour(side):
    """a wall of cost across the first tile's columns between the goal and the cells below it: crossing it costs 252 per step, the way round
    through the neighbouring tile (the whole way at cost 1) is cheaper -- the cheapest path leaves the tile and comes back"""
    edge = min(TILE, side - 3)
    cost = np.ones((side, side), np.int32)
    cost[TILE // 2 if side > TILE else side // 2, :edge] = 252
    goals = open_map(side)
    goals[3, 3] = 0
    return goals, None, cost, (min(side - 1, TILE - 2), 3)


def corner_goals(side):
    """goals on the corners of the tiles and of the map, and one on a blocked cell"""
    goals, blocked = open_map(side), open_map(side)
    marks = sorted({0, side - 1} | {v for k in range(1, (side - 1) // TILE + 1) for v in (k * TILE - 1, k * TILE)})
    rng = np.random.default_rng(side)
    for r in marks:
        for c in marks:
            if rng.random() < 0.4 or (r, c) in ((0, 0), (side - 1, side - 1)):
                goals[r, c] = 0
    blocked[side // 2, :] = 7
    blocked[side // 2, side // 3] = -1
    goals[side // 2, 1] = 0
    cost = (1 + (np.add.outer(np.arange(side), 2 * np.arange(side)) % 9)).astype(np.int32)
    return goals, blocked, cost, (side // 2 + 1, side // 2)


def pocket(side):
    """a walled-in pocket without a goal, with the start inside"""
    goals, blocked = open_map(side), open_map(side)
    a, b = side // 4, side // 2
    blocked[a, a:b + 1] = blocked[b, a:b + 1] = blocked[a:b + 1, a] = blocked[a:b + 1, b] = 0
    goals[side - 1, 0] = 0
    return goals, blocked, None, (a + 1, a + 1)


def no_goal(side):
    _, blocked, cost, start = random_field(side, 77)
    return open_map(side), blocked, cost, start


def all_blocked(side):
    goals = open_map(side)
    goals[1, 1] = goals[side - 2, 2] = 0
    return goals, np.zeros((side, side), np.int32), None, (1, 1)


def symmetric(side):
    """an open map around one goal: equal-cost ties in every octant decide the direction order"""
    goals = open_map(side)
    goals[side // 2, side // 2] = 0
    return goals, None, None, (0, side // 3)


SCENES = {"random": lambda side: random_field(side, 1000 + side, n_goals=3), "serpentine": serpentine, "detour": detour, "corners": corner_goals, "pocket": pocket,
          "no_goal": no_goal, "all_blocked": all_blocked, "symmetric": symmetric}


@functools.lru_cache(maxsize=None)
def scene(name, side):
    return SCENES[name](side)


@functools.lru_cache(maxsize=None)
def wanted(name, side, order, max_path, **kw):
    """the expectation of a scene, computed once and shared (nothing changes it)"""
    goals, blocked, cost, start = scene(name, side)
    p = route_ref.params(**kw)
    return route_ref.expected_routes(goals, blocked, cost, p, ORDER[order], route_ref.linear(*start, side, side, ORDER[order]), max_path, SIGNED_SENTINEL)


def filled(plane, side, fill):
    return plane if plane is not None else np.full((side, side), fill, np.int32)


def run_scenes(seg, names, order, tag, max_path=40, give=("next", "counts"), with_starts=True, slacks=(5, 2, 9, 3), **kw):
    """one call on the named scenes, sentinel-filled destinations and a stride of its own per buffer, compared with the reference map by map.
    A scene without a blocked (cost) plane gets an all-negative (all-one) one: the planes of a call are given for every map or for none"""
    import torch

    side, n, cells = seg.rows, len(names), seg.rows * seg.cols
    got = [scene(name, side) for name in names]
    strides = [cells + s for s in slacks]
    d_goals = pack([g[0] for g in got], ORDER[order], strides[0])
    d_blocked = pack([filled(g[1], side, -1) for g in got], ORDER[order], strides[1])
    d_cost = pack([filled(g[2], side, 1) for g in got], ORDER[order], strides[2])
    dst = Dest(n, strides[3], max_path, slack=131)
    starts = [route_ref.linear(*g[3], side, side, ORDER[order]) for g in got] if with_starts else None
    p = route_ref.params(**kw)
    rc = raw_route(seg, n, dst, d_goals, strides[0], d_blocked, strides[1], d_cost, strides[2], p, order, give, starts)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    wants = [wanted(name, side, order, max_path, **kw) for name in names]
    for i, w in enumerate(wants):
        check_map(host, i, w, order, dst, f"{tag}: {names[i]}", give, with_starts)
    check_tail(host, dst, tag)
    return wants


# ---------------------------------------------------------------- 1. the scenes at every side, in both orders

@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("side", [20, 67, 128])
def test_scenes(contexts, side, order):
    seg = contexts(side)
    first = run_scenes(seg, ["random", "serpentine", "detour", "corners", "symmetric"], order, f"scenes {side} {ORDER[order]}")
    second = run_scenes(seg, ["pocket", "no_goal", "all_blocked"], order, f"scenes {side} {ORDER[order]}")
    w = dict(zip(["random", "serpentine", "detour", "corners", "symmetric", "pocket", "no_goal", "all_blocked"], first + second))
    # the scenes hold what the test is about (on the expectation)
    corridors = (side + 1) // 2
    assert w["serpentine"]["path_len"] == corridors * side + corridors - 1  # every cell of every corridor and every gap between two
    assert w["serpentine"]["path_len"] > 40 and (w["serpentine"]["path"] != SIGNED_SENTINEL).all()  # truncated at max_path
    assert 0 < w["random"]["counts"][1] < w["random"]["counts"][2] < side * side and w["random"]["counts"][0] >= 1
    assert w["pocket"]["path_len"] == 0 and (w["pocket"]["dist"] == NONE).sum() > 4 and w["pocket"]["counts"][1] > side
    assert w["no_goal"]["counts"][:2].tolist() == [0, 0] and (w["no_goal"]["dist"] == NONE).all() and (w["no_goal"]["next"] == -1).all()
    assert w["all_blocked"]["counts"].tolist() == [0, 0, 0] and w["all_blocked"]["path_len"] == 0
    assert w["corners"]["counts"][0] >= 3 and w["symmetric"]["counts"].tolist() == [1, side * side, side * side]
    if side > TILE:  # the cheapest path of the detour leaves the first tile and comes back
        cells = [route_ref.cell_of(int(c), side, side, ORDER[order]) for c in w["detour"]["whole_path"]]
        assert cells[0][1] < TILE and cells[-1][1] < TILE and max(c[1] for c in cells) >= TILE


def test_both_orders_give_the_same_logical_result():
    """(on the expectations the device was just compared with) D does not depend on the order, and d_next names the same cell in both"""
    side = 67
    for name in ("random", "corners", "symmetric"):
        a, b = wanted(name, side, ROW, 40), wanted(name, side, COL, 40)
        assert np.array_equal(a["dist"], b["dist"]) and a["counts"].tolist() == b["counts"].tolist() and a["path_len"] == b["path_len"]
        rr, cc = np.nonzero(a["next"] >= 0)
        assert len(rr) > side
        for r, c in zip(rr[::7], cc[::7]):
            assert route_ref.cell_of(int(a["next"][r, c]), side, side, "row") == route_ref.cell_of(int(b["next"][r, c]), side, side, "col")


# ---------------------------------------------------------------- 2. connectivity, step weights, max_cost

@pytest.mark.parametrize("side", [67, 128])
def test_connectivity_4_and_other_weights(contexts, side):
    seg = contexts(side)
    run_scenes(seg, ["random", "serpentine", "symmetric"], ROW, f"four {side}", connectivity=4)
    run_scenes(seg, ["detour", "corners", "symmetric"], COL, f"weights {side}", straight=2, diagonal=3, cost_max=9)
    run_scenes(seg, ["symmetric", "random"], ROW, f"ties {side}", straight=1, diagonal=1, cost_max=1)  # every nearer neighbour attains the minimum


@pytest.mark.parametrize("side", [67, 128])
def test_max_cost(contexts, side):
    seg = contexts(side)
    free = wanted("symmetric", side, ROW, 40)
    R = int(np.median(free["dist"]))
    got = run_scenes(seg, ["symmetric", "random", "detour"], ROW, f"max_cost {side}", max_cost=R)
    keep = free["dist"] <= R
    assert 0 < keep.sum() < side * side and np.array_equal(got[0]["dist"], np.where(keep, free["dist"], NONE)) and got[0]["counts"][1] == keep.sum()
    assert got[0]["path_len"] == 0  # the start lies beyond R
    run_scenes(seg, ["symmetric", "random"], COL, f"max_cost 1 {side}", max_cost=1)  # the goals alone


# ---------------------------------------------------------------- 3. nullable inputs and outputs, n = 1

def test_null_inputs_and_outputs(contexts):
    import torch

    side = 67
    seg = contexts(side)
    cells = side * side
    goals, blocked, cost, start = scene("random", side)
    d_goals, d_blocked, d_cost = pack([goals], "row", cells + 1), pack([blocked], "row", cells + 4), pack([cost], "row", cells + 2)
    start = route_ref.linear(*start, side, side, "row")
    p = route_ref.params()
    for tag, b, c in (("no blocked", None, cost), ("no cost", blocked, None), ("neither", None, None)):
        dst = Dest(1, cells + 3, 16, slack=9)
        rc = raw_route(seg, 1, dst, d_goals, cells + 1, d_blocked if b is not None else 0, cells + 4 if b is not None else 0, d_cost if c is not None else 0,
                       cells + 2 if c is not None else 0, p, ROW, starts=[start])
        assert rc == 0, seg._L.gg_last_error(seg._ctx)
        torch.cuda.synchronize()
        host = dst.host()
        check_map(host, 0, route_ref.expected_routes(goals, b, c, p, "row", start, 16, SIGNED_SENTINEL), ROW, dst, tag)
        check_tail(host, dst, tag)
    for give, with_starts in (((), True), (("next",), True), (("counts",), True), (("next", "counts"), False), ((), False)):
        run_scenes(seg, ["random"], ROW, f"give {give} {with_starts}", give=give, with_starts=with_starts)


# ---------------------------------------------------------------- 4. past the ring, twice the same, streams

def test_past_the_ring_back_to_back(contexts):
    """PARAM_RING + 3 calls on one caller stream without a synchronisation, every one with other scenes, starts and order"""
    import torch

    side = 20
    seg = contexts(side)
    cells = side * side
    names = list(SCENES)
    calls = []
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for k in range(PARAM_RING + 3):
            pick = [names[(k + j) % len(names)] for j in range(4)]
            order = (ROW, COL)[k % 2]
            got = [scene(name, side) for name in pick]
            planes = [pack([filled(g[j], side, (-1, -1, 1)[j]) for g in got], ORDER[order], cells) for j in range(3)]
            dst = Dest(4, cells, 40)
            starts = [route_ref.linear(*g[3], side, side, ORDER[order]) for g in got]
            assert raw_route(seg, 4, dst, planes[0], cells, planes[1], cells, planes[2], cells, None, order, starts=starts) == 0, seg._L.gg_last_error(seg._ctx)
            calls.append((pick, order, planes, dst))
    torch.cuda.synchronize()
    for k, (pick, order, _, dst) in enumerate(calls):
        host = dst.host()
        for i, name in enumerate(pick):
            check_map(host, i, wanted(name, side, order, 40), order, dst, f"call {k}: {name}")


def test_twice_the_same(contexts):
    import torch

    side = 128
    seg = contexts(side)
    cells = side * side
    got = [scene(name, side) for name in ("random", "serpentine", "corners", "detour", "pocket")]
    planes = [pack([filled(g[j], side, (-1, -1, 1)[j]) for g in got], "col", cells + 1 + j) for j in range(3)]
    starts = [route_ref.linear(*g[3], side, side, "col") for g in got]
    runs = [Dest(5, cells + 7, 33), Dest(5, cells + 7, 33)]
    for dst in runs:
        assert raw_route(seg, 5, dst, planes[0], cells + 1, planes[1], cells + 2, planes[2], cells + 3, None, COL, starts=starts) == 0
    torch.cuda.synchronize()
    a, b = runs[0].host(), runs[1].host()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{key} differs between two runs"
    assert (a["counts"][:15] > 0).all()


def test_on_a_caller_stream_and_on_the_contexts_own(contexts):
    import torch

    side = 20
    seg = contexts(side)
    cells = side * side
    got = [scene(name, side) for name in ("random", "corners")]
    planes = [pack([filled(g[j], side, (-1, -1, 1)[j]) for g in got], "row", cells) for j in range(3)]
    starts = [route_ref.linear(*g[3], side, side, "row") for g in got]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    mine, own = Dest(2, cells, 40), Dest(2, cells, 40)
    assert raw_route(seg, 2, mine, planes[0], cells, planes[1], cells, planes[2], cells, starts=starts, stream=stream.cuda_stream) == 0
    stream.synchronize()
    assert raw_route(seg, 2, own, planes[0], cells, planes[1], cells, planes[2], cells, starts=starts, own=True) == 0
    seg.synchronize()
    for dst, tag in ((mine, "caller stream"), (own, "own stream")):
        host = dst.host()
        for i, name in enumerate(("random", "corners")):
            check_map(host, i, wanted(name, side, ROW, 40), ROW, dst, f"{tag}: {name}")


# ---------------------------------------------------------------- 5. nothing else changes

def test_nothing_changes():
    import torch

    side, K = 67, 3
    length, res = GEOMETRY[side]
    segs = [api.GroundSegmentation().init(length, res, n_slots=K, max_points=MAX_POINTS) for _ in range(2)]
    clouds = [[scan_cloud(9300 + k, (0.0, 0.0)) for k in range(K)], [scan_cloud(9310 + k, (0.6, -0.4)) for k in range(K)]]
    pts = [batch_points(c, MAX_POINTS) for c in clouds]
    n_pts = [[len(c) for c in batch] for batch in clouds]
    origins, base_z = np.zeros((2, 3), np.float32), np.full(2, -1.73)
    lazy = ["maxGroundHeight", "groundCandidates", "planeDist"]
    got = [scene(name, side) for name in ("random", "corners", "serpentine")]
    planes = [pack([filled(g[j], side, (-1, -1, 1)[j]) for g in got], "row", side * side).view(K, side, side) for j in range(3)]
    results = []
    for which, seg in enumerate(segs):
        seg.reset_maps(odom_z=0.1)
        seg.set_scoring(slots=[0, 1])
        seg.move_maps([(0.7, -0.4), (0.0, 0.4)], [POSE] * 2)
        seg.filter_batch(pts[0][:2].contiguous(), n_pts[0][:2], origins, base_z, slots=[0, 1], want_masks=True)  # (map 2 stays fresh)
        assert lazy_count(seg) == 2 and fresh_count(seg) == 1
        if which == 0:  # the calls between the two batches, on as many planes as the context has maps
            first = seg.route_planes(planes[0], planes[1], planes[2], on_torch_stream=True)
            seg.route_planes(planes[0], order="col", starts=[0, -1, 5], max_path=9, connectivity=4, on_torch_stream=True)
            assert lazy_count(seg) == 2 and fresh_count(seg) == 1
        pending = seg.export_layers(lazy, slots=[0, 1])
        assert lazy_count(seg) == 0
        after = seg.filter_batch(pts[1][:2].contiguous(), n_pts[1][:2], origins, base_z, slots=[0, 1])
        layers = seg.export_layers()
        torch.cuda.synchronize()
        if which == 0:
            assert first.counts.tolist() == [wanted(name, side, ROW, 40)["counts"].tolist() for name in ("random", "corners", "serpentine")]
        results.append(dict(fresh=fresh_count(seg), pending=pending.cpu().numpy(), planes=layers.cpu().numpy(), labels=after.labels.cpu().numpy(),
                            counts=after.counts.cpu().numpy(), scores=seg.scores_raw(), positions=[seg.map(s).getPosition() for s in range(K)]))
    a, b = results
    assert a["fresh"] == b["fresh"] == 1
    assert same_bits(a["pending"], b["pending"]) and same_bits(a["planes"], b["planes"]) and a["planes"].shape[1] == 11
    assert np.array_equal(a["counts"], b["counts"]) and a["positions"] == b["positions"]
    for k in range(2):
        assert np.array_equal(a["labels"][k, : n_pts[1][k]], b["labels"][k, : n_pts[1][k]])
    assert np.array_equal(a["scores"][0], b["scores"][0]) and np.array_equal(a["scores"][1], b["scores"][1]) and a["scores"][0].sum() == 4
    for seg in segs:
        seg.close()


# ---------------------------------------------------------------- 6. errors change nothing

def test_errors_change_nothing(contexts):
    import torch

    side = 20
    seg = contexts(side)
    cells, n = side * side, 3
    stride = cells + 8
    got = [scene(name, side) for name in ("random", "corners", "pocket")]
    d_goals, d_blocked, d_cost = (pack([filled(g[j], side, (-1, -1, 1)[j]) for g in got], "row", stride) for j in range(3))
    before = [t.clone() for t in (d_goals, d_blocked, d_cost)]
    dst = Dest(n, stride, 12)
    fresh_before, lazy_before = fresh_count(seg), lazy_count(seg)

    def call(n=n, goals=d_goals, goal_stride=stride, blocked=d_blocked, blocked_stride=stride, cost=d_cost, cost_stride=stride, order=ROW, starts=(0, -1, 7), **kw):
        p = dict(route_ref.DEFAULTS)
        p.update({k: kw.pop(k) for k in list(kw) if k in p})
        return raw_route(seg, n, dst, goals, goal_stride, blocked, blocked_stride, cost, cost_stride, p, order, starts=starts, **kw)

    x = _lib.GGPlaneRoutes()
    x.n = n
    assert seg._L.gg_route_planes(None, C.byref(x), None) == INVALID
    assert seg._L.gg_route_planes(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(goals=0) == INVALID
    assert call(dist=0) == INVALID
    assert call(goal_stride=cells - 1) == INVALID
    assert call(blocked_stride=cells - 1) == INVALID
    assert call(cost_stride=cells - 1) == INVALID
    assert call(plane_stride=cells - 1) == INVALID
    assert call(order=2) == INVALID
    assert call(order=-1) == INVALID
    for bad in (0, 5, 6, 9, -8):
        assert call(connectivity=bad) == INVALID
    for name in ("straight", "diagonal"):
        assert call(**{name: 0}) == INVALID
        assert call(**{name: 65536}) == INVALID
        assert call(**{name: -3}) == INVALID
    assert call(cost_max=0) == INVALID
    assert call(cost_max=-1) == INVALID
    assert call(max_cost=-1) == INVALID
    top = (2 ** 31 - 2) // (7 * cells)  # the overflow limit at its edge
    assert call(cost_max=top + 1) == INVALID
    assert call(straight=65535, diagonal=65535, cost_max=2 ** 31 - 1) == INVALID
    assert call(starts=(0, 1, 2), paths=0) == INVALID
    assert call(starts=(0, 1, 2), path_len=0) == INVALID
    assert call(starts=(0, 1, 2), max_path=0) == INVALID
    assert call(starts=(0, 1, 2), max_path=-4) == INVALID
    assert call(starts=(0, -2, 2)) == INVALID
    assert call(starts=(0, cells, 2)) == INVALID
    assert call(n=6, starts=(0,) * 6) == CAPACITY  # (more maps than the context has)
    # each pair of buffers that may not overlap: an output with an input, an output with another output
    buffers = dict(dist=dst.dist, next=dst.next)
    for name, t in buffers.items():
        for inp in (d_goals, d_blocked, d_cost):
            assert call(**{name: inp}) == INVALID, name
            assert call(**{name: inp.data_ptr() + 4 * ((n - 1) * stride + cells - 1)}) == INVALID, name  # (the last cell of the last plane)
        for other, u in buffers.items():
            if other != name:
                assert call(**{name: u}) == INVALID, (name, other)
    for name in ("counts", "paths", "path_len"):
        assert call(**{name: d_goals}) == INVALID, name
        assert call(**{name: d_cost.data_ptr() + 4 * stride}) == INVALID, name
        assert call(**{name: dst.dist.data_ptr() + 4 * (stride + 3)}) == INVALID, name
        assert call(**{name: dst.next}) == INVALID, name
    assert call(counts=dst.path_len) == INVALID
    assert call(paths=dst.counts) == INVALID
    assert call(path_len=dst.paths.data_ptr() + 4 * 5) == INVALID
    assert call(dist=dst.counts.data_ptr() - 4 * ((n - 1) * stride + cells - 1)) == INVALID  # (its last cell is the first count)
    assert call(n=0, goals=0, goal_stride=0, order=9, dist=0, plane_stride=0, connectivity=5, straight=-5, cost_max=0, starts=None) == 0  # n == 0: nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel() and all(torch.equal(t, b) for t, b in zip((d_goals, d_blocked, d_cost), before))
    assert fresh_count(seg) == fresh_before and lazy_count(seg) == lazy_before
    # ... and the same arguments without a mistake are accepted, at the edge of the limit too; the inputs may be one buffer; without starts the
    # path arguments are not looked at
    assert call() == 0, seg._L.gg_last_error(seg._ctx)
    assert call(cost_max=top) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(connectivity=4, diagonal=0, cost_max=(2 ** 31 - 2) // (5 * cells)) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(blocked=d_goals, cost=d_goals) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(starts=None, paths=0, path_len=0, max_path=0) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert not dst.all_sentinel()


# ---------------------------------------------------------------- 7. the chain on real data

def test_the_chain_from_a_drive(contexts):
    """three frames on two maps: move, filter, trace, fuse, then route_planes(goals=frontier, blocked=fused) from the robot cell, every call
    of a frame on one stream without a synchronisation between them; the planes of the last frame are downloaded and held against route_ref"""
    import torch

    side, K = 128, 2
    seg = contexts(side, n_slots=K)
    seg.reset_maps(odom_z=0.0)
    fuse = dict(hit=4, miss=3, decay=0, free_threshold=-2, occ_threshold=4)  # one free observation frees a cell
    track = np.array([[(0.0, 0.0), (0.0, 0.0)], [(1.1, -0.8), (-0.5, 0.4)], [(2.5, -0.9), (-1.9, 1.5)]])
    robot = route_ref.linear(side // 2, side // 2, side, side, "row")
    evidence, outs = None, [api.FusionOutputs(), api.FusionOutputs()]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for f in range(len(track)):
            shifts = seg.move_maps(track[f], [POSE] * K, on_torch_stream=True)
            clouds = [scan_cloud(9500 + 10 * f + k, track[f, k]) for k in range(K)]
            stride = stride_of(clouds)
            pts, n_pts = batch_points(clouds, stride), [len(c) for c in clouds]
            origins = np.concatenate([track[f], np.full((K, 1), 1.7)], axis=1).astype(np.float32)
            out = seg.filter_batch(pts, n_pts, origins, np.full(K, -1.73), want_masks=True)
            vis = seg.visibility_clouds(pts, n_pts, origins, masks=out.label_masks, min_height=0.2, max_height=3.0)
            fused = seg.fuse_states(vis.state, evidence, shifts=shifts, out=outs[f % 2], on_torch_stream=True, **fuse)
            evidence = fused.evidence
            routes = seg.route_planes(fused.frontier, fused.state, starts=[robot] * K, max_path=2 * side, on_torch_stream=True)
    torch.cuda.synchronize()
    frontier, state = fused.frontier.cpu().numpy(), fused.state.cpu().numpy()
    assert (frontier == 0).sum() > 20 and (state < 0).sum() > 300  # a frontier to route to and free space to cross
    reached = 0
    for k in range(K):
        want = route_ref.expected_routes(frontier[k], state[k], None, None, "row", robot, 2 * side, -1)
        assert np.array_equal(routes.dist[k].cpu().numpy(), want["dist"]) and np.array_equal(routes.next[k].cpu().numpy(), want["next"]), f"map {k}"
        assert routes.counts[k].tolist() == want["counts"].tolist() and int(routes.path_len[k].item()) == want["path_len"], f"map {k}"
        assert np.array_equal(routes.paths[k].cpu().numpy(), want["path"]), f"map {k}"
        assert want["counts"][0] == (frontier[k] == 0).sum()  # (a frontier cell is free: every one is a goal)
        reached += want["counts"][1] - want["counts"][0]
    assert reached > 50  # cells that are no goals were routed


# ---------------------------------------------------------------- 8. the headline shape

def test_headline_shape(contexts):
    """two random fields of 364 x 364: 6 x 6 tiles, the last 44 cells wide"""
    import torch

    side, n = 364, 2
    seg = contexts(side, n_slots=2)
    cells = side * side
    fields = [random_field(side, 3640 + i, n_goals=1 + 2 * i) for i in range(n)]
    planes = [pack([f[j] for f in fields], "row", cells) for j in range(3)]
    starts = [route_ref.linear(*f[3], side, side, "row") for f in fields]
    dst = Dest(n, cells, 64, slack=17)
    assert raw_route(seg, n, dst, planes[0], cells, planes[1], cells, planes[2], cells, None, ROW, starts=starts) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    for i, f in enumerate(fields):
        want = route_ref.expected_routes(f[0], f[1], f[2], None, "row", starts[i], 64, SIGNED_SENTINEL)
        assert want["counts"][1] > cells // 2
        check_map(host, i, want, ROW, dst, f"headline: map {i}")
    check_tail(host, dst, "headline")


# ---------------------------------------------------------------- 9. the Python entry point

def test_python_entry_point(contexts):
    import torch

    side, names = 20, ("random", "corners", "pocket", "symmetric")
    n = len(names)
    seg = contexts(side)
    got = [scene(name, side) for name in names]
    d_goals, d_blocked, d_cost = (pack([filled(g[j], side, (-1, -1, 1)[j]) for g in got], "row", side * side).view(n, side, side) for j in range(3))
    starts = [route_ref.linear(*g[3], side, side, "row") for g in got]
    a = seg.route_planes(d_goals, d_blocked, d_cost, starts=starts, max_path=40, on_torch_stream=True)
    assert isinstance(a, api.RouteOutputs)
    for t, shape in ((a.dist, (n, side, side)), (a.next, (n, side, side)), (a.counts, (n, 3)), (a.paths, (n, 40)), (a.path_len, (n,))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    b = seg.route_planes(d_goals, d_blocked, d_cost, next=False, counts=False, on_torch_stream=True)
    assert b.next is None and b.counts is None and b.paths is None and b.path_len is None
    col_starts = [route_ref.linear(*g[3], side, side, "col") for g in got]
    c = seg.route_planes(*(t.transpose(1, 2).contiguous() for t in (d_goals, d_blocked, d_cost)), order="col", starts=np.array(col_starts), max_path=40, on_torch_stream=True)
    cell_goals = api.goal_planes([[(3, 4), (19, 0)], [], [(0, 0)], [(7, 7)]], side, side, device="cuda")
    d = seg.route_planes(cell_goals, connectivity=4, straight=3, on_torch_stream=True)
    torch.cuda.synchronize()
    for i, name in enumerate(names):
        want, want_col = wanted(name, side, ROW, 40), wanted(name, side, COL, 40)
        assert np.array_equal(a.dist[i].cpu().numpy(), want["dist"]) and np.array_equal(a.next[i].cpu().numpy(), want["next"])
        assert a.counts[i].tolist() == want["counts"].tolist() and int(a.path_len[i].item()) == want["path_len"]
        assert np.array_equal(a.paths[i].cpu().numpy(), np.where(want["path"] == SIGNED_SENTINEL, -1, want["path"]))  # (allocated by the call: -1 behind the path)
        assert np.array_equal(b.dist[i].cpu().numpy(), want["dist"])
        assert np.array_equal(c.dist[i].cpu().numpy(), want_col["dist"].T) and np.array_equal(c.next[i].cpu().numpy(), want_col["next"].T)
        assert int(c.path_len[i].item()) == want_col["path_len"]
        open_want = route_ref.expected_routes(cell_goals[i].cpu().numpy(), None, None, route_ref.params(connectivity=4, straight=3))
        assert np.array_equal(d.dist[i].cpu().numpy(), open_want["dist"]) and d.counts[i].tolist() == open_want["counts"].tolist()
    # out= is reused and written; the context's own stream is the default
    a.dist.fill_(SIGNED_SENTINEL)
    a.counts.fill_(SIGNED_SENTINEL)
    torch.cuda.synchronize()
    again = seg.route_planes(d_goals, d_blocked, d_cost, starts=starts, max_path=40, out=a)
    assert again is a
    seg.synchronize()
    assert np.array_equal(a.dist.cpu().numpy(), np.stack([wanted(name, side, ROW, 40)["dist"] for name in names]))
    assert a.counts.tolist() == [wanted(name, side, ROW, 40)["counts"].tolist() for name in names]
    with pytest.raises(ValueError):  # no update in place
        seg.route_planes(d_goals, out=api.RouteOutputs(dist=d_goals))
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, d_blocked, out=api.RouteOutputs(next=d_blocked))
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, counts=False, out=a)  # (counts, paths that are not asked for)
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, out=api.RouteOutputs(dist=torch.empty((n, side, side + 1), dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError):
        seg.route_planes(d_goals.to(torch.int64))
    with pytest.raises(ValueError):
        seg.route_planes(d_goals[:, :, :19])
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, d_blocked[:2])
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, cost=d_cost.to(torch.int64))
    for bad in (starts[:3], [starts], [0.5] * n, "left", [side * side] * n, [-2] * n):
        with pytest.raises(ValueError):
            seg.route_planes(d_goals, starts=bad, max_path=8)
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, starts=starts)  # (max_path)
    with pytest.raises(ValueError):
        seg.route_planes(d_goals, straight=0)
    with pytest.raises(api.GroundGridError):  # more planes than the context has maps: the library's GG_ERR_CAPACITY
        seg.route_planes(torch.cat([d_goals, d_goals]))
