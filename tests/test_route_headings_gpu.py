"""gg_route_headings (the cost-to-go over cells and headings, the moves and the paths of many maps over a heading mask, in device memory) on the
device.  Expected values come from numpy alone (tests/headings_ref.py: a binary-heap Dijkstra over the reversed moves, held against
Bellman-Ford sweeps and scipy's Dijkstra by tests/test_route_headings_cpu.py).  Every comparison is on bits: every word of d_dist, d_next,
d_best and d_best_heading, the counts, the path rows and lengths, the words between a plane and its stride and behind the last plane.
The library's maps are square, so the sides 23 and 41 stand where a 23 x 41 map would: a transposed move table or swapped sides show on a
square map as well, because no scene here and no table is its own transpose."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402
from tests import footprint_ref, route_ref  # noqa: E402
from tests import headings_ref as ref  # noqa: E402
from tests.test_export_layers_gpu import POSE, batch_points, fresh_count, same_bits, stride_of  # noqa: E402
from tests.test_fuse_states_gpu import MAX_POINTS, SIGNED_SENTINEL, pack, scan_cloud  # noqa: E402
from tests.test_split_clouds_gpu import PARAM_RING, lazy_count  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
NONE, ANY = ref.NONE, ref.ANY
GEOMETRY = {20: (7.0, 0.35), 23: (8.0, 0.348), 37: (12.0, 0.325), 41: (14.0, 0.3415), 67: (22.0, 0.33), 364: (120.0, 0.33)}  # side: (length, resolution)
VOLUMES = ("dist", "next")        # K planes per map
PLANES = ("best", "best_heading")  # one plane per map
NULLABLE = ("next", "best", "best_heading", "counts")


# ---------------------------------------------------------------- helpers

@pytest.fixture(scope="module")
def contexts():
    """one context per (side, slots), made on demand and shared: no call of this file but the drive's changes a map"""
    made = {}

    def get(side, n_slots=8):
        if (side, n_slots) not in made:
            length, res = GEOMETRY[side]
            seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=MAX_POINTS)
            assert seg.rows == seg.cols == side
            made[(side, n_slots)] = seg
        return made[(side, n_slots)]

    yield get
    for seg in made.values():
        seg.close()


class Dest:
    """sentinel-filled destinations of one call, every buffer with strides of its own and a few words behind"""

    def __init__(self, n, K, cells, max_len=1, slacks=(5, 2, 9, 3, 4)):
        import torch

        def filled(words):
            return torch.full((max(words, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

        self.n, self.K, self.cells, self.max_len = n, K, cells, max_len
        self.plane_stride, self.next_plane_stride = cells + slacks[0], cells + slacks[1]
        self.dist_stride, self.next_stride = K * self.plane_stride + slacks[2], K * self.next_plane_stride + slacks[3]
        self.best_stride, self.best_heading_stride = cells + slacks[3], cells + slacks[4]
        self.path_stride = 2 * max_len + slacks[1]
        self.dist, self.next = filled(n * self.dist_stride + 11), filled(n * self.next_stride + 7)
        self.best, self.best_heading = filled(n * self.best_stride + 6), filled(n * self.best_heading_stride + 5)
        self.counts, self.paths, self.path_len = filled(3 * n + 3), filled(n * self.path_stride + 5), filled(n + 3)

    NAMES = ("dist", "next", "best", "best_heading", "counts", "paths", "path_len")

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in self.NAMES}

    def all_sentinel(self):
        return all(bool((getattr(self, k) == SIGNED_SENTINEL).all().item()) for k in self.NAMES)


def raw_headings(seg, n, dest, mask, mask_stride, goals, goal_stride, moves, cost=None, cost_stride=0, goal_headings=ANY, cost_max=252, max_cost=0,
                 order=ROW, give=NULLABLE, starts=None, stream=None, own=False, **over):
    """gg_route_headings as the C ABI has it (mask, goals, cost: device tensors or addresses, 0 / None = null; moves: [K, 8, 4] or None;
    starts: [n, 2] or None); returns the status.  `give`: the nullable outputs handed over; `over`: any field of the struct in place of
    what follows from `dest`"""
    import torch

    def address(t):
        return (t.data_ptr() if torch.is_tensor(t) else t) or None

    x = _lib.GGHeadingRoutes()
    x.n, x.d_mask, x.mask_stride, x.d_goals, x.goal_stride = n, address(mask), mask_stride, address(goals), goal_stride
    x.d_cost, x.cost_stride = address(cost), cost_stride
    host_moves = None
    if moves is not None:
        host_moves = np.ascontiguousarray(np.asarray(moves, np.int32))
        x.moves = host_moves.ctypes.data_as(C.POINTER(C.c_int32))
    x.n_headings = over.get("n_headings", host_moves.shape[0] if host_moves is not None else dest.K)
    x.goal_headings, x.cost_max, x.max_cost, x.order = goal_headings, cost_max, max_cost, order
    x.d_dist = address(over.get("dist", dest.dist))
    x.d_next = address(over.get("next", dest.next if "next" in give else 0))
    x.d_best = address(over.get("best", dest.best if "best" in give else 0))
    x.d_best_heading = address(over.get("best_heading", dest.best_heading if "best_heading" in give else 0))
    x.d_counts = address(over.get("counts", dest.counts if "counts" in give else 0))
    for k in ("dist_stride", "plane_stride", "next_stride", "next_plane_stride", "best_stride", "best_heading_stride", "path_stride", "max_len"):
        setattr(x, k, over.get(k, getattr(dest, k)))
    st = None
    if starts is not None:
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1, 2))
        x.starts = st.ctypes.data_as(C.POINTER(C.c_int32))
    x.d_paths, x.d_path_len = address(over.get("paths", dest.paths)), address(over.get("path_len", dest.path_len))
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_route_headings(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check_map(host, i, want, order, dest, tag, give=NULLABLE, with_paths=True):
    """map i of a downloaded Dest against headings_ref.expected_headings: every word of every given plane, the counts, the path row and
    length, the words between a plane and its stride and between the last plane of a map and the next map, and what was not handed over"""
    K, cells = dest.K, dest.cells
    for name, stride, plane_stride in (("dist", dest.dist_stride, dest.plane_stride), ("next", dest.next_stride, dest.next_plane_stride)):
        words = host[name][i * stride: (i + 1) * stride]
        if name != "dist" and name not in give:
            assert np.all(words == SIGNED_SENTINEL), f"{tag}: map {i}: {name} was not handed over and was written"
            continue
        for k in range(K):
            plane = ref.lay(want[name][k], ORDER[order]).ravel()
            got = words[k * plane_stride: (k + 1) * plane_stride]
            bad = np.flatnonzero(got[:cells] != plane)
            assert len(bad) == 0, f"{tag}: map {i}: {name}, heading {k}: {len(bad)} words differ, first at {bad[0]}: {got[bad[0]]} != {plane[bad[0]]}"
            assert np.all(got[cells:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words between plane {k} of {name} and its stride were written"
        assert np.all(words[K * plane_stride:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words behind the last {name} plane of the map were written"
    for name, stride in (("best", dest.best_stride), ("best_heading", dest.best_heading_stride)):
        words = host[name][i * stride: (i + 1) * stride]
        if name not in give:
            assert np.all(words == SIGNED_SENTINEL), f"{tag}: map {i}: {name} was not handed over and was written"
            continue
        plane = ref.lay(want[name], ORDER[order]).ravel()
        bad = np.flatnonzero(words[:cells] != plane)
        assert len(bad) == 0, f"{tag}: map {i}: {name}: {len(bad)} words differ, first at {bad[0]}: {words[bad[0]]} != {plane[bad[0]]}"
        assert np.all(words[cells:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words behind the {name} plane were written"
    counts = host["counts"][3 * i: 3 * i + 3]
    if "counts" in give:
        assert counts.tolist() == want["counts"].tolist(), f"{tag}: map {i}: counts {counts} != {want['counts']}"
    else:
        assert np.all(counts == SIGNED_SENTINEL), f"{tag}: map {i}: the counts were not handed over and were written"
    row, length = host["paths"][i * dest.path_stride: (i + 1) * dest.path_stride], host["path_len"][i]
    if with_paths:
        assert length == want["path_len"], f"{tag}: map {i}: path_len {length} != {want['path_len']}"
        assert np.array_equal(row[: 2 * dest.max_len].reshape(-1, 2), want["path"]), f"{tag}: map {i}: the path row differs"
        assert np.all(row[2 * dest.max_len:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words behind the path row were written"
    else:
        assert length == SIGNED_SENTINEL and np.all(row == SIGNED_SENTINEL), f"{tag}: map {i}: no starts were given and the paths were written"


def check_tail(host, dest, tag):
    n = dest.n
    for name, stride in (("dist", dest.dist_stride), ("next", dest.next_stride), ("best", dest.best_stride), ("best_heading", dest.best_heading_stride),
                         ("counts", 3), ("paths", dest.path_stride), ("path_len", 1)):
        assert np.all(host[name][n * stride:] == SIGNED_SENTINEL), f"{tag}: the words behind the last {name} were written"


# ---------------------------------------------------------------- scenes: (mask, goals, cost, start (r, c, k)) as logical [side, side] planes

def all_headings(side, K):
    return np.full((side, side), (1 << K) - 1, np.int64).astype(np.uint32).view(np.int32)


def no_goals(side):
    return np.full((side, side), -1, np.int32)


def open_corners(side, K):
    """everything admissible, goals on the corners and on the rim: most moves of the cells near them would leave the map"""
    goals = no_goals(side)
    goals[0, 0] = goals[side - 1, side - 1] = goals[0, side // 2] = goals[side - 1, 1] = 0
    return all_headings(side, K), goals, None, (side // 2, side // 3, K - 1)


def seams(side, K):
    """goals and walls on cells 0 .. 3 either side of every seam of the tiles, both ways, everything else admissible; costs that differ
    from cell to cell, so that a swapped side or a transposed offset shows"""
    T = _lib.headings_tile(K)
    rng = np.random.default_rng(side * 64 + K)
    near = sorted({v for s in range(T, side, T) for v in range(s - 4, s + 4) if 0 <= v < side}) or list(range(side // 2 - 4, side // 2 + 4))  # (a map of one tile: its middle)
    mask, goals = all_headings(side, K).copy(), no_goals(side)
    for v in near:
        for u in range(0, side):
            for r, c in ((v, u), (u, v)):
                p = rng.random()
                if p < 0.25:
                    mask[r, c] = 0
                elif p < 0.29:
                    goals[r, c] = 0
    goals[near[0], near[-1]] = 0
    mask[near[0], near[-1]] = -1
    cost = (1 + (np.add.outer(3 * np.arange(side), 7 * np.arange(side)) % 11)).astype(np.int32)
    return mask, goals, cost, (side - 1, 0, 0)


def serpentine(side, K):
    """corridors one cell wide along the even rows, joined at alternating ends, every heading admissible inside: with one-cell moves and
    turns in place the chain from the last corridor to the goal at (0, 0) walks every one of them, leaving and re-entering the same tiles"""
    mask = all_headings(side, K).copy()
    for r in range(1, side, 2):
        mask[r, :] = 0
        mask[r, side - 1 if (r // 2) % 2 == 0 else 0] = -1
    goals = no_goals(side)
    goals[0, 0] = 0
    last = (side - 1) // 2 * 2
    return mask, goals, None, (last, side - 1 if (last // 2) % 2 == 0 else 0, 0)


def no_goal(side, K):
    mask, _, cost, start = ref.random_scene(side, K, 77)
    return mask, no_goals(side), cost, start


def nothing_admissible(side, K):
    goals = no_goals(side)
    goals[1, 1] = goals[side - 2, 2] = 0
    mask = np.zeros((side, side), np.int64)
    if K < 32:
        mask[:] = ((1 << 32) - 1) & ~((1 << K) - 1)  # (every bit above K is set: they are ignored)
    return mask.astype(np.uint32).view(np.int32), goals, None, (1, 1, 0)


def dead_end(side, K):
    return ref.dead_end(side, K)[:4]


SCENES = {"random": lambda side, K: ref.random_case(side, K)[:4], "dead_end": dead_end, "open": open_corners, "seams": seams, "serpentine": serpentine,
          "no_goal": no_goal, "nothing": nothing_admissible}


@functools.lru_cache(maxsize=None)
def scene(name, side, K):
    return SCENES[name](side, K)


def start_of(name, side, K, order, want):
    """the start pose of a scene: the reached state with the dearest way where there is one (its path is the longest), the scene's own where
    nothing is reached"""
    D = want["dist"]
    r, c, k = scene(name, side, K)[3]
    if (D != NONE).any():
        k, r, c = np.unravel_index(np.argmax(np.where(D == NONE, -1, D)), D.shape)
    return (ref.linear(int(r), int(c), side, side, ORDER[order]), int(k))


TABLES = {}


def table_of(key, K):
    """the move tables of this file by name: the helper's at steps 1 .. 3 with and without reverse and turns in place, and a hand-made one with
    an asymmetric 3-cell move, absent entries in the middle and a turn in place one way only"""
    if (key, K) not in TABLES:
        if key == "hand":
            t = np.zeros((K, 8, 4), np.int32)
            for k in range(K):
                t[k, 0] = (-3, 1, k, 31)
                t[k, 2] = (1, -2, (k + 1) % K, 17)
                t[k, 5] = (0, 1, (k + K - 1) % K, 9)
                if K > 1:
                    t[k, 7] = (0, 0, (k + 1) % K, 4)
        elif key == "four":
            t = np.array([[(-1, 0, 0, 5), (0, -1, 0, 5), (0, 1, 0, 5), (1, 0, 0, 5)] + [(0, 0, 0, 0)] * 4], np.int32)
        else:
            step, pct, spin = key
            t = ref.table(K, step, 10, turn=3, reverse_pct=pct, spin=spin)
        assert ref.moves_ok(t, K)
        TABLES[(key, K)] = t
    return TABLES[(key, K)]


@functools.lru_cache(maxsize=None)
def unbounded(name, side, K, key, goal_headings):
    """the expectation of a scene without a start, computed once and shared (nothing changes it)"""
    mask, goals, cost, _ = scene(name, side, K)
    moves = ref.random_table(side, K) if key == "random" else table_of(key, K)
    return ref.expected_headings(mask, goals, cost, moves, goal_headings)


@functools.lru_cache(maxsize=None)
def wanted(name, side, K, key, order, max_len, goal_headings=ANY, max_cost=0):
    mask, goals, cost, _ = scene(name, side, K)
    moves = ref.random_table(side, K) if key == "random" else table_of(key, K)
    start = start_of(name, side, K, order, unbounded(name, side, K, key, goal_headings))
    return ref.expected_headings(mask, goals, cost, moves, goal_headings, max_cost=max_cost, order=ORDER[order], start=start, max_len=max_len, sentinel=SIGNED_SENTINEL), start


def filled(plane, side, fill):
    return plane if plane is not None else np.full((side, side), fill, np.int32)


def run_scenes(seg, names, K, key, order, tag, max_len=40, give=NULLABLE, with_starts=True, with_cost=True, goal_headings=ANY, max_cost=0, **kw):
    """one call on the named scenes, sentinel-filled destinations and a stride of its own per buffer, compared with the reference map by map.
    A scene without a cost plane gets an all-one plane: the planes of a call are given for every map or for none"""
    import torch

    side, n, cells = seg.rows, len(names), seg.rows * seg.cols
    got = [scene(name, side, K) for name in names]
    moves = ref.random_table(side, K) if key == "random" else table_of(key, K)
    strides = [cells + 6, cells + 1, cells + 10]
    d_mask = pack([g[0] for g in got], ORDER[order], strides[0])
    d_goals = pack([g[1] for g in got], ORDER[order], strides[1])
    d_cost = pack([filled(g[2], side, 1) for g in got], ORDER[order], strides[2]) if with_cost else None
    assert with_cost or all(g[2] is None for g in got)
    wants = [wanted(name, side, K, key, order, max_len, goal_headings, max_cost) for name in names]
    dst = Dest(n, K, cells, max_len)
    starts = [w[1] for w in wants] if with_starts else None
    rc = raw_headings(seg, n, dst, d_mask, strides[0], d_goals, strides[1], moves, d_cost, strides[2] if with_cost else 0, goal_headings, 252, max_cost, order,
                      give, starts, **kw)
    assert rc == 0, f"{tag}: {seg._L.gg_last_error(seg._ctx)}"
    if kw.get("own"):
        seg.synchronize()
    torch.cuda.synchronize()
    host = dst.host()
    for i, name in enumerate(names):
        check_map(host, i, wants[i][0], order, dst, f"{tag}: {name}", give, with_starts)
    check_tail(host, dst, tag)
    return dst, [w[0] for w in wants]


# ---------------------------------------------------------------- 1. the scenes of one call, on bits, at every side, K and order

@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("side", [20, 23, 37, 41, 67])
def test_scenes_of_one_call(contexts, side, K, order):
    """the random mask of (side, K) under its own helper table (steps 1 .. 3, with and without reverse and turns in place across the set),
    the dead end, goals on the rim of an open map, the seams, no goal and nothing admissible: six maps of one call"""
    _, wants = run_scenes(contexts(side), ("random", "dead_end", "open", "seams", "no_goal", "nothing"), K, "random", order, f"{side} K={K} {ORDER[order]}")
    assert ref.scene_classes(wants[0], ref.random_table(side, K))[1] >= 100
    assert np.all(wants[4]["dist"] == NONE) and np.all(wants[5]["dist"] == NONE) and wants[5]["counts"].tolist() == [0, 0, 0]
    assert wants[2]["counts"][2] == K * side * side  # everything admissible


@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("side,K,key", [(37, 8, "hand"), (37, 32, "hand"), (67, 16, "hand"), (67, 32, (3, 150, 0)), (67, 8, (3, 0, 7)), (20, 16, "hand"),
                                        (41, 32, (2, 150, 9))])
def test_three_cell_moves_across_the_seams(contexts, side, K, key, order):
    """goals and walls on cells 0 .. 3 either side of every seam (at 32 up to 16 headings, at 16 above; a last tile of 5 or 3 cells, narrower
    than the halo, at 37 and 67), under the hand-made table and the helper's longest moves"""
    _, wants = run_scenes(contexts(side), ("seams", "open", "random"), K, key, order, f"seams {side} K={K} {key}")
    assert (wants[0]["dist"] != NONE).sum() > side * side


@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("side,K", [(37, 8), (67, 8), (37, 32)])
def test_serpentine_and_the_heading_wrap(contexts, side, K, order):
    """one-cell moves with turns in place: the serpentine's chain leaves and re-enters every tile; on the open map the cheapest chains turn
    through the wrap between heading 0 and heading K - 1 both ways"""
    key = (1, 0, 4)
    _, wants = run_scenes(contexts(side), ("serpentine", "open"), K, key, order, f"serpentine {side} K={K}", max_len=2 * side * side, with_cost=False)
    assert wants[0]["path_len"] > side * side // 2
    moves, nxt, D = table_of(key, K), wants[1]["next"], wants[1]["dist"]
    for k, k2 in ((0, K - 1), (K - 1, 0)):
        slots = [m for m in range(8) if moves[k, m, 3] and moves[k, m, 2] == k2]
        assert np.isin(nxt[k][(D[k] != NONE) & (D[k] > 0)], slots).any(), (k, k2)


def test_one_goal_heading_max_cost_and_n_one(contexts):
    side, K = 37, 16
    seg = contexts(side)
    key = (2, 150, 0)
    run_scenes(seg, ("random", "open", "seams"), K, key, ROW, "goal heading 5", goal_headings=1 << 5)
    run_scenes(seg, ("random", "open"), K, key, COL, "goal headings above K alone", goal_headings=0xFFFF0000)
    finite = unbounded("random", side, K, key, ANY)["dist"]
    median = int(np.median(finite[finite != NONE]))
    for R in (median, 1):
        _, wants = run_scenes(seg, ("random", "open", "seams"), K, key, ROW, f"max_cost {R}", max_cost=R)
        assert wants[0]["counts"][1] < unbounded("random", side, K, key, ANY)["counts"][1]
    run_scenes(seg, ("random",), K, key, COL, "n = 1")
    run_scenes(seg, ("open",), 1, "four", ROW, "n = 1, K = 1", with_cost=False)


@pytest.mark.parametrize("side", [20, 67])
def test_one_heading_and_four_moves_equal_route_planes(contexts, side):
    """K = 1 with the four unit moves and the mask "not blocked": gg_route_planes at connectivity 4 on the same planes, word for word"""
    import torch

    seg = contexts(side)
    cells = side * side
    rng = np.random.default_rng(side)
    blocked = np.where(rng.random((3, side, side)) < 0.3, 2, -1).astype(np.int32)
    cost = rng.integers(-3, 300, (3, side, side)).astype(np.int32)
    goals = np.where(rng.random((3, side, side)) < 0.01, 0, -1).astype(np.int32)
    d_blocked, d_cost, d_goals = (torch.from_numpy(a).cuda() for a in (blocked, cost, goals))
    d_mask = (d_blocked < 0).to(torch.int32)
    flat = seg.route_planes(d_goals, d_blocked, d_cost, connectivity=4, straight=5, on_torch_stream=True)
    deep = seg.route_headings(d_mask, d_goals, table_of("four", 1), d_cost, on_torch_stream=True)
    torch.cuda.synchronize()
    assert torch.equal(deep.dist[:, 0], flat.dist) and torch.equal(deep.best, flat.dist) and torch.equal(deep.counts, flat.counts)
    step = torch.tensor([-side, -1, 1, side, 0, 0, 0, 0, 0], device="cuda")
    index = torch.arange(cells, device="cuda").view(1, side, side)
    slot = deep.next[:, 0].long()
    assert torch.equal(torch.where(slot < 0, -1, index + step[slot.clamp(min=0)]).to(torch.int32), flat.next)
    for i in range(3):
        want = ref.expected_headings(d_mask[i].cpu().numpy(), goals[i], cost[i], table_of("four", 1))
        assert np.array_equal(deep.dist[i].cpu().numpy(), want["dist"]) and np.array_equal(deep.next[i].cpu().numpy(), want["next"])
    assert int((flat.dist != NONE).sum()) > 100


@pytest.mark.parametrize("name", ["dead_end", "l_bend"])
def test_purpose_scenes(contexts, name):
    """the dead end whose goal heading looks back out and the narrow L-bend: unreached forwards, reached with reverse moves"""
    import torch

    side = 20
    seg = contexts(side)
    mask, goals, _, (r0, c0, k0), gh = ref.dead_end(side) if name == "dead_end" else ref.l_bend(side)
    K = 8 if name == "dead_end" else 4
    d_mask, d_goals = torch.from_numpy(np.stack([mask, mask])).cuda(), torch.from_numpy(np.stack([goals, goals])).cuda()
    starts = [(r0 * side + c0, k0)] * 2
    for pct, reached in ((0, False), (150, True)):
        moves = ref.table(K, 1, 10, turn=2, reverse_pct=pct)
        out = seg.route_headings(d_mask, d_goals, moves, goal_headings=gh, starts=starts, max_len=64, on_torch_stream=True)
        torch.cuda.synchronize()
        want = ref.expected_headings(mask, goals, None, moves, gh, start=starts[0], max_len=64, sentinel=-1)
        for i in range(2):
            assert np.array_equal(out.dist[i].cpu().numpy(), want["dist"]) and np.array_equal(out.next[i].cpu().numpy(), want["next"])
            assert np.array_equal(out.paths[i].cpu().numpy(), want["path"]) and int(out.path_len[i]) == want["path_len"]
        assert (int(out.dist[0, k0, r0, c0]) != NONE) == reached == (want["path_len"] > 0)


# ---------------------------------------------------------------- 2. the nullable outputs, the ring, determinism, the streams

def test_every_subset_of_the_nullable_outputs(contexts):
    seg = contexts(20)
    for r in range(len(NULLABLE) + 1):
        for give in itertools.combinations(NULLABLE, r):
            for with_starts in (False, True):
                run_scenes(seg, ("random", "open"), 8, (1, 150, 5), ROW if r % 2 else COL, f"give {give}, starts {with_starts}", give=give, with_starts=with_starts)


def test_more_calls_than_the_ring_has_entries_and_two_runs(contexts):
    """PARAM_RING + 3 calls back to back, each with a table, starts and goal headings of its own, nothing synchronised in between: every
    call's outputs are its own; the whole sequence again gives the same bytes"""
    import torch

    side, K, names = 37, 8, ("random", "seams", "open")
    seg = contexts(side)
    cells = side * side
    keys = [(1, 0, 0), "hand", (2, 150, 0), (3, 0, 6), (1, 150, 3), (2, 0, 0), (3, 150, 9)][: PARAM_RING + 3]
    assert len(keys) == PARAM_RING + 3
    got = [scene(name, side, K) for name in names]
    d_mask, d_goals = pack([g[0] for g in got], "row", cells), pack([g[1] for g in got], "row", cells)
    d_cost = pack([filled(g[2], side, 1) for g in got], "row", cells)
    runs = []
    for _ in range(2):
        dests = [Dest(len(names), K, cells, 30) for _ in keys]
        for j, key in enumerate(keys):
            starts = [wanted(name, side, K, key, ROW, 30, 1 << j)[1] for name in names]
            assert raw_headings(seg, len(names), dests[j], d_mask, cells, d_goals, cells, table_of(key, K), d_cost, cells, 1 << j, starts=starts) == 0
        torch.cuda.synchronize()
        runs.append([d.host() for d in dests])
        for j, key in enumerate(keys):
            for i, name in enumerate(names):
                check_map(runs[-1][j], i, wanted(name, side, K, key, ROW, 30, 1 << j)[0], ROW, dests[j], f"call {j}: {name}")
            check_tail(runs[-1][j], dests[j], f"call {j}")
    for a, b in zip(*runs):
        assert all(a[k].tobytes() == b[k].tobytes() for k in Dest.NAMES)


def test_a_callers_stream_and_the_contexts_own(contexts):
    import torch

    seg = contexts(41)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        run_scenes(seg, ("random", "seams"), 16, "random", ROW, "caller stream", stream=stream.cuda_stream)
    run_scenes(seg, ("random", "seams"), 16, "random", COL, "own stream", own=True)


# ---------------------------------------------------------------- 3. no map changes

def test_no_map_changes():
    """a context with two filtered maps and a fresh one: the lazy and fresh counters, the positions and an exported layer are the same
    before and after"""
    import torch

    side, n = 67, 3
    length, res = GEOMETRY[side]
    seg = api.GroundSegmentation().init(length, res, n_slots=n, max_points=MAX_POINTS)
    clouds = [scan_cloud(9400 + k, (0.0, 0.0)) for k in range(2)]
    pts, n_pts = batch_points(clouds, MAX_POINTS), [len(c) for c in clouds]
    seg.reset_maps(odom_z=0.1)
    seg.move_maps([(0.7, -0.4), (0.0, 0.4)], [POSE] * 2)
    seg.filter_batch(pts, n_pts, np.zeros((2, 3), np.float32), np.full(2, -1.73), slots=[0, 1])  # (map 2 stays fresh)
    assert lazy_count(seg) == 2 and fresh_count(seg) == 1
    layer_before = seg.export_layers(["ground"]).cpu().numpy()
    counters = (lazy_count(seg), fresh_count(seg))
    positions = [seg.map(s).getPosition() for s in range(n)]
    names, K, key = ("random", "seams", "open"), 8, (2, 150, 0)
    got = [scene(name, side, K) for name in names]
    d_mask = torch.from_numpy(np.stack([g[0] for g in got])).cuda()
    d_goals = torch.from_numpy(np.stack([g[1] for g in got])).cuda()
    first = seg.route_headings(d_mask, d_goals, table_of(key, K), on_torch_stream=True)
    seg.route_headings(d_mask.transpose(1, 2).contiguous(), d_goals.transpose(1, 2).contiguous(), table_of("hand", K), order="col", on_torch_stream=True)
    assert (lazy_count(seg), fresh_count(seg)) == counters
    layer_after = seg.export_layers(["ground"]).cpu().numpy()
    torch.cuda.synchronize()
    assert (lazy_count(seg), fresh_count(seg)) == counters and positions == [seg.map(s).getPosition() for s in range(n)]
    assert same_bits(layer_before, layer_after) and np.isfinite(layer_before).any()
    for i, g in enumerate(got):
        assert first.counts[i].tolist() == ref.expected_headings(g[0], g[1], None, table_of(key, K))["counts"].tolist()
    seg.close()


# ---------------------------------------------------------------- 4. errors change nothing

def test_errors_change_nothing(contexts):
    import torch

    side, K, n, names = 20, 8, 3, ("random", "seams", "open")
    seg = contexts(side, n_slots=5)
    cells = side * side
    stride = cells + 8
    moves = table_of((1, 150, 5), K)
    got = [scene(name, side, K) for name in names]
    d_mask, d_goals = pack([g[0] for g in got], "row", stride), pack([g[1] for g in got], "row", stride)
    d_cost = pack([filled(g[2], side, 1) for g in got], "row", stride)
    before = [t.clone() for t in (d_mask, d_goals, d_cost)]
    dst = Dest(n, K, cells, 10)
    fresh_before, lazy_before = fresh_count(seg), lazy_count(seg)
    good_starts = [(5, 1), (-1, 99), (cells - 1, K - 1)]

    def call(n=n, mask=d_mask, mask_stride=stride, goals=d_goals, goal_stride=stride, moves=moves, cost=d_cost, cost_stride=stride, starts=good_starts, **kw):
        return raw_headings(seg, n, dst, mask, mask_stride, goals, goal_stride, moves, cost, cost_stride, starts=starts, **kw)

    def changed(k, m, entry):
        t = moves.copy()
        t[k, m] = entry
        return t

    x = _lib.GGHeadingRoutes()
    x.n = n
    assert seg._L.gg_route_headings(None, C.byref(x), None) == INVALID
    assert seg._L.gg_route_headings(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(mask=0) == INVALID and call(goals=0) == INVALID and call(dist=0) == INVALID
    assert call(moves=None, n_headings=K) == INVALID
    for bad in (0, -1, 33):
        assert call(n_headings=bad) == INVALID, bad
    assert call(mask_stride=cells - 1) == INVALID and call(goal_stride=cells - 1) == INVALID and call(cost_stride=cells - 1) == INVALID
    assert call(plane_stride=cells - 1) == INVALID and call(dist_stride=K * dst.plane_stride - 1) == INVALID
    assert call(next_plane_stride=cells - 1) == INVALID and call(next_stride=K * dst.next_plane_stride - 1) == INVALID
    assert call(best_stride=cells - 1) == INVALID and call(best_heading_stride=cells - 1) == INVALID
    assert call(order=2) == INVALID and call(order=-1) == INVALID
    assert call(cost_max=0) == INVALID and call(cost_max=-5) == INVALID and call(max_cost=-1) == INVALID
    # every bad move word; an absent entry may hold anything
    for entry in ((1, 0, 0, 32768), (1, 0, 0, -1), (4, 0, 0, 5), (0, -4, 0, 5), (1, 0, K, 5), (1, 0, -1, 5), (0, 0, 2, 5), (-2 ** 31, 0, 0, 5)):
        assert call(moves=changed(2, 3, entry)) == INVALID, entry
    # the overflow limit at its edge: s * cost_max * cells * K, s = 32767 in one entry
    dear = changed(0, 0, (1, 0, 0, 32767))
    at_limit = ref.LIMIT // (32767 * cells * K)
    assert call(moves=dear, cost_max=at_limit + 1) == INVALID and call(moves=dear, cost_max=2 ** 31 - 1) == INVALID
    # the starts
    assert call(paths=0) == INVALID and call(path_len=0) == INVALID and call(max_len=0) == INVALID and call(path_stride=2 * dst.max_len - 1) == INVALID
    for bad in ((-2, 0), (cells, 0), (3, K), (3, -1)):
        assert call(starts=[good_starts[0], bad, good_starts[2]]) == INVALID, bad
    assert call(n=6, starts=None) == CAPACITY  # (more maps than the context has)
    # each pair of buffers that may not overlap: an output with an input, the outputs with each other
    last_in = 4 * ((n - 1) * stride + cells - 1)
    last = {"dist": 4 * ((n - 1) * dst.dist_stride + (K - 1) * dst.plane_stride + cells - 1), "next": 4 * ((n - 1) * dst.next_stride + (K - 1) * dst.next_plane_stride + cells - 1),
            "best": 4 * ((n - 1) * dst.best_stride + cells - 1), "best_heading": 4 * ((n - 1) * dst.best_heading_stride + cells - 1), "counts": 4 * (3 * n - 1),
            "paths": 4 * ((n - 1) * dst.path_stride + 2 * dst.max_len - 1), "path_len": 4 * (n - 1)}
    small = {"counts", "paths", "path_len"}
    for name in Dest.NAMES:
        for src in (d_mask, d_goals, d_cost):
            if name not in small:
                assert call(**{name: src}) == INVALID, name
            assert call(**{name: src.data_ptr() + last_in}) == INVALID, name  # (the last cell of the input's last plane)
    for a, b in itertools.permutations(Dest.NAMES, 2):
        assert call(**{a: getattr(dst, b).data_ptr() + last[b]}) == INVALID, (a, b)  # (the last word the other output may write)
    assert call(n=0, mask=0, goals=0, moves=None, order=9, cost_max=-4, n_headings=99, starts=None) == 0  # n == 0: nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel() and all(torch.equal(a, b) for a, b in zip((d_mask, d_goals, d_cost), before))
    assert fresh_count(seg) == fresh_before and lazy_count(seg) == lazy_before
    # ... and the same arguments without a mistake are accepted, at the edges of the ranges too
    assert call() == 0, seg._L.gg_last_error(seg._ctx)
    assert call(moves=dear, cost_max=at_limit, order=COL) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(moves=changed(2, 3, (99, -99, 77, 0))) == 0, seg._L.gg_last_error(seg._ctx)  # (an absent entry of any words)
    assert call(starts=None, paths=0, path_len=0, max_len=0, path_stride=0) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(give=(), next_stride=0, next_plane_stride=0, best_stride=0, best_heading_stride=0) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert not dst.all_sentinel()


# ---------------------------------------------------------------- 5. the chain on real data

def test_the_chain_from_a_drive(contexts):
    """three frames on two maps: move, filter, trace, fuse, then footprint_planes(fused state) and route_headings(mask, goals = the frontier),
    every call on one stream; the mask is held to footprint_ref and every output of route_headings to headings_ref on that mask"""
    import torch

    side, n, K = 67, 2, 8
    seg = contexts(side, n_slots=n)
    seg.reset_maps(odom_z=0.0)
    track = np.array([[(0.0, 0.0), (0.0, 0.0)], [(1.1, -0.8), (-0.5, 0.4)], [(2.5, -0.9), (-1.9, 1.5)]])
    rotations = api.rotation_table([2.0 * np.pi * k / K for k in range(K)])
    spans = api.footprint_spans(rotations, 2.0, 0.0, 0.5, 0.5, pad=0.3, radius=3)
    moves = api.heading_moves(rotations, step=1, unit=10, turn=3, reverse_pct=200)
    assert np.array_equal(moves, ref.table(K, 1, 10, turn=3, reverse_pct=200))
    evidence, outs, log = None, [api.FusionOutputs(), api.FusionOutputs()], []
    fuse = dict(hit=4, miss=3, free_threshold=-2, occ_threshold=4)  # (one miss makes a cell free: free cells from the first frame on)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for f in range(len(track)):
            shifts = seg.move_maps(track[f], [POSE] * n, on_torch_stream=True)
            clouds = [scan_cloud(9800 + 10 * f + k, track[f, k]) for k in range(n)]
            stride = stride_of(clouds)
            pts, n_pts = batch_points(clouds, stride), [len(c) for c in clouds]
            origins = np.concatenate([track[f], np.full((n, 1), 1.7)], axis=1).astype(np.float32)
            out = seg.filter_batch(pts, n_pts, origins, np.full(n, -1.73), want_masks=True)
            vis = seg.visibility_clouds(pts, n_pts, origins, masks=out.label_masks, min_height=0.2, max_height=3.0)
            fused = seg.fuse_states(vis.state, evidence, shifts=np.array(shifts), out=outs[f % 2], on_torch_stream=True, **fuse)
            evidence = fused.evidence
            fits = seg.footprint_planes(fused.state, spans, min_fit=1, outside_free=True, fit=False, counts=False, on_torch_stream=True)
            starts = [((side // 2) * side + side // 2, 0)] * n
            routes = seg.route_headings(fits.mask, fused.frontier, moves, starts=starts, max_len=50, on_torch_stream=True)
            log.append(dict(state=fused.state.clone(), frontier=fused.frontier.clone(), mask=fits.mask, routes=routes, starts=starts))
    torch.cuda.synchronize()
    reached = 0
    for f, e in enumerate(log):
        for k in range(n):
            mask = footprint_ref.expected_footprint(e["state"][k].cpu().numpy(), spans, 1, 1)["mask"]
            assert np.array_equal(e["mask"][k].cpu().numpy().view(np.uint32), mask), f"frame {f}, map {k}"
            want = ref.expected_headings(mask.view(np.int32), e["frontier"][k].cpu().numpy(), None, moves, start=e["starts"][k], max_len=50, sentinel=-1)
            r = e["routes"]
            for name in ("dist", "next", "best", "best_heading", "counts"):
                assert np.array_equal(getattr(r, name)[k].cpu().numpy(), want[name]), f"frame {f}, map {k}: {name}"
            assert int(r.path_len[k]) == want["path_len"] and np.array_equal(r.paths[k].cpu().numpy(), want["path"]), f"frame {f}, map {k}"
            reached += int(want["counts"][1] - want["counts"][0])
    assert reached > 1000


# ---------------------------------------------------------------- 6. the Python entry point

def test_python_entry_point(contexts):
    import torch

    side, K, names = 23, 8, ("random", "seams", "open")
    n = len(names)
    seg = contexts(side)
    got = [scene(name, side, K) for name in names]
    d_mask, d_goals = torch.from_numpy(np.stack([g[0] for g in got])).cuda(), torch.from_numpy(np.stack([g[1] for g in got])).cuda()
    d_cost = torch.from_numpy(np.stack([filled(g[2], side, 1) for g in got])).cuda()
    moves = table_of((2, 150, 0), K)
    a = seg.route_headings(d_mask, d_goals, moves, d_cost, on_torch_stream=True)
    assert isinstance(a, api.HeadingOutputs) and a.paths is None and a.path_len is None
    for t, shape in ((a.dist, (n, K, side, side)), (a.next, (n, K, side, side)), (a.best, (n, side, side)), (a.best_heading, (n, side, side)), (a.counts, (n, 3))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    starts = [(side + 1, 0), (-1, 0), (5 * side + 7, 3)]
    b = seg.route_headings(d_mask, d_goals, moves.tolist(), d_cost, goal_headings=0b110, max_cost=400, next=False, best=False, counts=False, starts=starts,
                           max_len=12, on_torch_stream=True)
    assert b.next is None and b.best is None and b.best_heading is None and b.counts is None and tuple(b.paths.shape) == (n, 12, 2)
    tr = [t.transpose(1, 2).contiguous() for t in (d_mask, d_goals, d_cost)]
    col_starts = [(ref.linear(*ref.cell_of(c, side, side, "row"), side, side, "col") if c >= 0 else -1, k) for c, k in starts]
    c = seg.route_headings(tr[0], tr[1], moves, tr[2], order="col", starts=col_starts, max_len=12, on_torch_stream=True)
    again = seg.route_headings(d_mask, d_goals, moves, d_cost, out=a)
    assert again is a
    seg.synchronize()
    torch.cuda.synchronize()
    for i, g in enumerate(got):
        want = ref.expected_headings(g[0], g[1], filled(g[2], side, 1), moves)
        for name in ("dist", "next", "best", "best_heading", "counts"):
            assert np.array_equal(getattr(a, name)[i].cpu().numpy(), want[name]), (i, name)
        assert np.array_equal(c.dist[i].cpu().numpy(), want["dist"].transpose(0, 2, 1)) and np.array_equal(c.best_heading[i].cpu().numpy(), want["best_heading"].T)
        cut = ref.expected_headings(g[0], g[1], filled(g[2], side, 1), moves, 0b110, max_cost=400, start=starts[i], max_len=12, sentinel=-1)
        assert np.array_equal(b.dist[i].cpu().numpy(), cut["dist"]) and np.array_equal(b.paths[i].cpu().numpy(), cut["path"]) and int(b.path_len[i]) == cut["path_len"]
        col = ref.expected_headings(g[0], g[1], filled(g[2], side, 1), moves, order="col", start=col_starts[i], max_len=12, sentinel=-1)
        assert np.array_equal(c.paths[i].cpu().numpy(), col["path"]) and int(c.path_len[i]) == col["path_len"]
    # bad arguments are refused before the call
    bad_calls = [dict(out=api.HeadingOutputs(dist=torch.zeros_like(a.dist), best=d_goals)), dict(next=False, out=a), dict(order="diagonal"), dict(cost_max=0),
                 dict(max_cost=-1), dict(goal_headings=-1), dict(max_len=3), dict(starts=[(0, 0)] * n), dict(starts=[(0, K)] * n, max_len=3),
                 dict(starts=[(side * side, 0)] * n, max_len=3), dict(cost_max=2 ** 31 - 1)]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            seg.route_headings(d_mask, d_goals, moves, d_cost, **kw)
    for bad_moves in (moves[:, :7], np.where(moves == moves[0, 0, 3], 40000, moves), np.where(moves == moves[0, 0, 0], 4, moves)):
        with pytest.raises(ValueError):
            seg.route_headings(d_mask, d_goals, bad_moves, d_cost)
    with pytest.raises(ValueError):
        seg.route_headings(d_mask.to(torch.int64), d_goals, moves)
    with pytest.raises(ValueError):
        seg.route_headings(d_mask, d_goals[:, :, :19], moves)
    with pytest.raises(api.GroundGridError):  # more planes than the context has maps: the library's GG_ERR_CAPACITY
        seg.route_headings(torch.cat([d_mask] * 3), torch.cat([d_goals] * 3), moves)


# ---------------------------------------------------------------- 7. one map of the size of the benchmark's

def test_a_map_of_364_cells_a_side():
    """one random mask of 364 x 364 at K = 16 under the helper's table of step 2 with reverse moves; the expectation by scipy's Dijkstra on
    the explicit graph (headings_ref.graph_cost_to_go, which the CPU tests hold equal to the heap search), next and best from that D"""
    import torch

    side, K = 364, 16
    length, res = GEOMETRY[side]
    seg = api.GroundSegmentation().init(length, res, n_slots=1, max_points=MAX_POINTS)
    assert seg.rows == seg.cols == side
    mask, goals, cost, _ = ref.random_scene(side, K, 364, density=0.25, n_goals=12)
    moves = ref.table(K, 2, 10, turn=3, reverse_pct=150)
    cost_max = ref.LIMIT // (int(moves[:, :, 3].max()) * side * side * K)  # the largest the overflow limit allows at this size
    assert cost_max == 26
    want = ref.expected_headings(mask, goals, cost, moves, cost_max=cost_max, search=ref.graph_cost_to_go)
    out = seg.route_headings(torch.from_numpy(mask[None]).cuda(), torch.from_numpy(goals[None]).cuda(), moves, torch.from_numpy(cost[None]).cuda(),
                             cost_max=cost_max, on_torch_stream=True)
    torch.cuda.synchronize()
    for name in ("dist", "next", "best", "best_heading", "counts"):
        assert np.array_equal(getattr(out, name)[0].cpu().numpy(), want[name]), name
    assert want["counts"][1] > 100000
    seg.close()
