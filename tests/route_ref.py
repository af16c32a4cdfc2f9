"""The definition of gg_route_planes (include/groundgrid_hip.h) restated with a binary-heap Dijkstra over numpy planes: D, next from the final
D by the direction order, the counts, the paths and max_cost.  No device and no library code: the GPU tests compare against this on bits,
and tests/test_route_planes_cpu.py holds it against two independent restatements (Bellman-Ford sweeps, scipy's Dijkstra on the graph)."""
import heapq

import numpy as np

NONE = 0x7FFFFFFF
# the direction order of d_next, in (row, col) terms: the four straight steps, then the four diagonals
DIRECTIONS = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))
DEFAULTS = dict(connectivity=8, straight=5, diagonal=7, cost_max=252, max_cost=0)  # those of GroundSegmentation.route_planes
LIMIT = 2 ** 31 - 2  # of max(straight, diagonal) * cost_max * rows * cols


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def within_limit(rows, cols, p):
    """the overflow limit of the header: what gg_route_planes accepts"""
    s = max(p["straight"], p["diagonal"] if p["connectivity"] == 8 else 0)
    ok = 1 <= p["straight"] <= 65535 and (p["connectivity"] == 4 or 1 <= p["diagonal"] <= 65535) and p["cost_max"] >= 1
    return ok and s * p["cost_max"] * rows * cols <= LIMIT


def lay(a, order):
    """a logical [rows, cols] array as the plane of `order`: [rows, cols] row-major, [cols, rows] column-major"""
    return np.ascontiguousarray(a if order == "row" else a.T)


def linear(r, c, rows, cols, order):
    """the linear index of cell (r, c) in a plane of `order`"""
    return r * cols + c if order == "row" else c * rows + r


def cell_of(index, rows, cols, order):
    return (index // cols, index % cols) if order == "row" else (index % rows, index // rows)


def blocked_of(blocked, shape):
    return np.zeros(shape, bool) if blocked is None else np.asarray(blocked).astype(np.int64) >= 0


def weights_of(cost, shape, p):
    return np.ones(shape, np.int64) if cost is None else np.minimum(np.maximum(np.asarray(cost).astype(np.int64), 1), p["cost_max"])


def cost_to_go(goals, blocked, cost, p):
    """the unbounded D of one map, int64 [rows, cols], NONE where no chain of admissible steps reaches a goal: Dijkstra from the goals.
    Leaving p for q along the reverse of the step q -> p costs s * w(p): the weight of the cell the PATH enters, which is the cell the
    search leaves.  (Plain lists over a plane with a blocked rim, so that no neighbour needs a bounds test: this is the slow part.)"""
    goals = np.asarray(goals)
    rows, cols = goals.shape
    B = blocked_of(blocked, goals.shape)
    pitch = cols + 2
    rim = np.ones((rows + 2, pitch), bool)
    rim[1:-1, 1:-1] = B
    closed = rim.ravel().tolist()
    w = np.zeros((rows + 2, pitch), np.int64)
    w[1:-1, 1:-1] = weights_of(cost, B.shape, p)
    w = w.ravel().tolist()
    moves = [(a * pitch + b, a * pitch, b, p["straight"] if k < 4 else p["diagonal"], k >= 4) for k, (a, b) in enumerate(DIRECTIONS[:p["connectivity"]])]
    D = [NONE] * len(closed)
    heap = []
    for r, c in np.argwhere((goals.astype(np.int64) >= 0) & ~B):
        at = (int(r) + 1) * pitch + int(c) + 1
        D[at] = 0
        heap.append((0, at))
    heapq.heapify(heap)
    while heap:
        d, at = heapq.heappop(heap)
        if d > D[at]:
            continue
        wp = w[at]
        for off, da, db, s, diagonal in moves:  # (being admissible is mutual, and so are the two side cells of a diagonal)
            q = at + off
            if closed[q] or (diagonal and (closed[at + da] or closed[at + db])):
                continue
            nd = d + s * wp
            if nd < D[q]:
                D[q] = nd
                heapq.heappush(heap, (nd, q))
    return np.array(D, np.int64).reshape(rows + 2, pitch)[1:-1, 1:-1].copy()


def next_of(D, blocked, cost, p, order):
    """d_next from a final (unbounded or masked) D: own index on a goal, -1 on an unreached cell, else the first direction of DIRECTIONS whose
    step is admissible and attains D(q) = D(p) + s * w(p).  Whole planes at a time, the directions from the last to the first so that the
    first one that attains stays"""
    rows, cols = D.shape
    B = blocked_of(blocked, D.shape)
    w = weights_of(cost, D.shape, p)
    rr, cc = np.mgrid[0:rows, 0:cols]

    def shifted(a, da, db, fill):
        """out[r, c] = a[r + da, c + db] where that cell exists, `fill` elsewhere"""
        out = np.full(a.shape, fill, a.dtype)
        rs, re, cs, ce = max(0, -da), min(rows, rows - da), max(0, -db), min(cols, cols - db)
        out[rs:re, cs:ce] = a[rs + da:re + da, cs + db:ce + db]
        return out

    nxt = np.full(D.shape, -1, np.int64)
    for k in reversed(range(p["connectivity"])):
        a, b = DIRECTIONS[k]
        ok = ~B & ~shifted(B, a, b, True)
        if k >= 4:
            ok &= ~shifted(B, a, 0, True) & ~shifted(B, 0, b, True)
        attains = ok & (shifted(D, a, b, NONE) + (p["straight"] if k < 4 else p["diagonal"]) * shifted(w, a, b, 0) == D)
        nxt = np.where(attains, linear(rr + a, cc + b, rows, cols, order), nxt)
    reached = D != NONE
    assert (nxt[reached & (D != 0)] >= 0).all(), "D is no fixed point"
    nxt = np.where(D == 0, linear(rr, cc, rows, cols, order), nxt)
    return np.where(reached, nxt, -1)


def path_from(start, D, nxt, order):
    """the cells of the path from linear index `start` (in `order`): [] for -1 or an unreached cell"""
    rows, cols = D.shape
    if start < 0:
        return []
    r, c = cell_of(start, rows, cols, order)
    if D[r, c] == NONE:
        return []
    path = [start]
    while D[r, c] != 0:
        here = int(nxt[r, c])
        assert here >= 0 and len(path) <= rows * cols
        path.append(here)
        r, c = cell_of(here, rows, cols, order)
    return path


def expected_routes(goals, blocked=None, cost=None, p=None, order="row", start=None, max_path=0, sentinel=0):
    """the definition for one map: goals, blocked, cost logical [rows, cols] (any int32 words; blocked and cost may be None).  Returns
    dict(dist, next: int32 [rows, cols], logical, next holding linear indices in `order`; counts: int32 [3] goals, reached, unblocked;
    path_len: int; path: int32 [max_path], `sentinel` where the call writes nothing)"""
    p = p or params()
    goals = np.asarray(goals)
    rows, cols = goals.shape
    assert within_limit(rows, cols, p)
    B = blocked_of(blocked, goals.shape)
    D = cost_to_go(goals, blocked, cost, p)
    assert D.max() <= NONE
    if p["max_cost"] > 0:
        D = np.where(D > p["max_cost"], NONE, D)
    nxt = next_of(D, blocked, cost, p, order)
    out = {"dist": D.astype(np.int32), "next": nxt.astype(np.int32),
           "counts": np.array([int((D == 0).sum()), int((D != NONE).sum()), int((~B).sum())], np.int32)}
    if start is not None:
        path = path_from(int(start), D, nxt, order)
        row = np.full(max_path, sentinel, np.int32)
        row[:min(len(path), max_path)] = path[:max_path]
        out["path"], out["path_len"], out["whole_path"] = row, len(path), path
    return out
