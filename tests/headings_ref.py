"""The definition of gg_route_headings and gg_heading_moves (include/groundgrid_hip.h) restated: a binary-heap Dijkstra over the reversed move
graph of (heading, cell) states gives D; next, best, the counts and the paths are taken from the final D by the header's tie rules; the
move table of the helper in plain Python integers.  No device and no library code: the GPU tests compare against this on bits, and
tests/test_route_headings_cpu.py holds it against two restatements that share no search with it (Bellman-Ford sweeps over the whole volume,
scipy's Dijkstra on the explicit graph -- graph_cost_to_go below, which the one large GPU test uses because it is fast)."""
import heapq
import math

import numpy as np

NONE = 0x7FFFFFFF
MAX_HEADINGS, MAX_MOVES, MAX_STEP, MAX_COST, AT_GOAL = 32, 8, 3, 32767, 8
LIMIT = 2 ** 31 - 2  # of max s * cost_max * rows * cols * K
UNIT = 16384
ANY = 0xFFFFFFFF


def lay(a, order):
    """a logical [rows, cols] array as the plane of `order`: [rows, cols] row-major, [cols, rows] column-major"""
    return np.ascontiguousarray(a if order == "row" else a.T)


def linear(r, c, rows, cols, order):
    return r * cols + c if order == "row" else c * rows + r


def cell_of(index, rows, cols, order):
    return (index // cols, index % cols) if order == "row" else (index % rows, index // rows)


# ---------------------------------------------------------------- gg_heading_moves

def rha(v):
    """v / 16384 rounded half away from zero"""
    return -((-v + UNIT // 2) >> 14) if v < 0 else (v + UNIT // 2) >> 14


def heading_moves(rotations, step, unit, turn, reverse_pct, spin):
    """the table [K][8][4] as nested lists of Python integers, or None where the header says GG_ERR_INVALID"""
    rot = [[int(v) for v in pair] for pair in rotations]
    K = len(rot)
    if not 1 <= K <= MAX_HEADINGS or any(abs(v) > UNIT for pair in rot for v in pair):
        return None
    if not (1 <= step <= MAX_STEP and 1 <= unit <= 1024 and turn >= 0 and spin >= 0 and (reverse_pct == 0 or reverse_pct >= 100)):
        return None
    table = [[[0, 0, 0, 0] for _ in range(MAX_MOVES)] for _ in range(K)]
    for k, (cq, sq) in enumerate(rot):
        da, db = rha(step * cq), rha(step * sq)
        left, right = (k + 1) % K, (k - 1) % K
        if (da, db) != (0, 0):
            s = max(1, math.isqrt(unit * unit * (da * da + db * db)))
            table[k][0] = [da, db, k, s]
            table[k][1] = [da, db, left, s + turn]
            table[k][2] = [da, db, right, s + turn]
            if reverse_pct:
                for m, (k2, c) in enumerate(((k, s), (left, s + turn), (right, s + turn))):
                    table[k][3 + m] = [-da, -db, k2, -((-c * reverse_pct) // 100)]
        if spin and K > 1:
            table[k][6] = [0, 0, left, spin]
            table[k][7] = [0, 0, right, spin]
    if any(e[3] > MAX_COST for row in table for e in row):
        return None
    return table


def rotations(K, offset=0.0):
    """K evenly spaced headings as the Q14 pairs api.rotation_table makes, restated: heading k looks along (cos, sin) of offset + 2 pi k / K"""
    out = []
    for k in range(K):
        a = offset + 2.0 * math.pi * k / K
        out.append([int(math.copysign(math.floor(abs(v) * UNIT + 0.5), v)) for v in (math.cos(a), math.sin(a))])
    return np.array(out, np.int32)


def table(K, step=1, unit=10, turn=0, reverse_pct=0, spin=0, offset=0.0):
    t = heading_moves(rotations(K, offset), step, unit, turn, reverse_pct, spin)
    assert t is not None
    return np.array(t, np.int32)


# ---------------------------------------------------------------- D

def moves_ok(moves, K):
    """the header's conditions on a move table"""
    moves = np.asarray(moves)
    if moves.shape != (K, MAX_MOVES, 4):
        return False
    for k in range(K):
        for da, db, k2, s in moves[k].tolist():
            if s == 0:
                continue
            if not (1 <= s <= MAX_COST and abs(da) <= MAX_STEP and abs(db) <= MAX_STEP and 0 <= k2 < K) or (da, db, k2) == (0, 0, k):
                return False
    return True


def within_limit(rows, cols, K, moves, cost_max):
    s_max = int(np.asarray(moves)[:, :, 3].max())
    return cost_max >= 1 and s_max * cost_max * rows * cols * K <= LIMIT


def admissible_of(mask, K):
    """bool [K, rows, cols] from the mask words (any int32 / uint32 words; bits K .. 31 are ignored)"""
    m = np.asarray(mask).astype(np.int64) & 0xFFFFFFFF
    return np.stack([((m >> k) & 1).astype(bool) for k in range(K)])


def weights_of(cost, shape, cost_max):
    return np.ones(shape, np.int64) if cost is None else np.minimum(np.maximum(np.asarray(cost).astype(np.int64), 1), cost_max)


def goal_states(mask, goals, K, goal_headings):
    adm = admissible_of(mask, K)
    wanted = np.array([(goal_headings >> k) & 1 for k in range(K)], bool)[:, None, None]
    return adm & wanted & (np.asarray(goals).astype(np.int64) >= 0)[None]


def cost_to_go(mask, goals, cost, moves, goal_headings=ANY, cost_max=252):
    """the unbounded D of one map, int64 [K, rows, cols]: Dijkstra from the goal states over the reversed moves.  Reaching (k, q) from
    (k2, p = q + d) along the reverse of the move costs s * w(p): the weight of the cell the PATH enters, which the search leaves.  (Plain
    lists over a volume with a rim of MAX_STEP inadmissible cells, so that no source needs a bounds test: this is the slow part.)"""
    moves = np.asarray(moves)
    K = moves.shape[0]
    rows, cols = np.asarray(goals).shape
    adm = admissible_of(mask, K)
    pitch, plane = cols + 2 * MAX_STEP, (rows + 2 * MAX_STEP) * (cols + 2 * MAX_STEP)
    A = np.zeros((K, rows + 2 * MAX_STEP, pitch), bool)
    A[:, MAX_STEP:-MAX_STEP, MAX_STEP:-MAX_STEP] = adm
    ok = A.ravel().tolist()
    W = np.zeros((rows + 2 * MAX_STEP, pitch), np.int64)
    W[MAX_STEP:-MAX_STEP, MAX_STEP:-MAX_STEP] = weights_of(cost, (rows, cols), cost_max)
    w = W.ravel().tolist()
    into = [[] for _ in range(K)]  # into[k2]: (offset from the target state to the source state, s) of every move that ends at heading k2
    for k in range(K):
        for da, db, k2, s in moves[k].tolist():
            if s:
                into[k2].append(((k - k2) * plane - da * pitch - db, s))
    D = [NONE] * (K * plane)
    heap = []
    G = np.zeros_like(A)
    G[:, MAX_STEP:-MAX_STEP, MAX_STEP:-MAX_STEP] = goal_states(mask, goals, K, goal_headings)
    for at in np.flatnonzero(G.ravel()).tolist():
        D[at] = 0
        heap.append((0, at))
    heapq.heapify(heap)
    while heap:
        d, at = heapq.heappop(heap)
        if d > D[at]:
            continue
        k2, p = divmod(at, plane)
        wp = w[p]
        for off, s in into[k2]:
            q = at + off
            if not ok[q]:
                continue
            nd = d + s * wp
            if nd < D[q]:
                D[q] = nd
                heapq.heappush(heap, (nd, q))
    return np.array(D, np.int64).reshape(K, rows + 2 * MAX_STEP, pitch)[:, MAX_STEP:-MAX_STEP, MAX_STEP:-MAX_STEP].copy()


def shifted(a, da, db, fill):
    """out[r, c] = a[r + da, c + db] where that cell exists, `fill` elsewhere"""
    rows, cols = a.shape
    out = np.full(a.shape, fill, a.dtype)
    rs, re, cs, ce = max(0, -da), min(rows, rows - da), max(0, -db), min(cols, cols - db)
    if rs < re and cs < ce:
        out[rs:re, cs:ce] = a[rs + da:re + da, cs + db:ce + db]
    return out


def edges_of(mask, cost, moves, cost_max):
    """every admissible move of one map as arrays (source state, target state, cost), states numbered (k * rows + r) * cols + c"""
    moves = np.asarray(moves)
    K = moves.shape[0]
    adm = admissible_of(mask, K)
    rows, cols = adm.shape[1:]
    w = weights_of(cost, (rows, cols), cost_max)
    cell = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    src, dst, val = [], [], []
    for k in range(K):
        for da, db, k2, s in moves[k].tolist():
            if not s:
                continue
            ok = adm[k] & shifted(adm[k2], da, db, False)
            src.append(k * rows * cols + cell[ok])
            dst.append(k2 * rows * cols + shifted(cell, da, db, 0)[ok])
            val.append(s * shifted(w, da, db, 0)[ok])
    if not src:
        return (np.zeros(0, np.int64),) * 3
    return np.concatenate(src), np.concatenate(dst), np.concatenate(val)


def graph_cost_to_go(mask, goals, cost, moves, goal_headings=ANY, cost_max=252):
    """D by scipy's Dijkstra on the explicit reversed graph (costs below 2^31 are exact in its float64)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra

    moves = np.asarray(moves)
    K = moves.shape[0]
    rows, cols = np.asarray(goals).shape
    n = K * rows * cols
    G = goal_states(mask, goals, K, goal_headings)
    sources = np.flatnonzero(G.ravel())
    D = np.full(n, NONE, np.int64)
    if len(sources):
        src, dst, val = edges_of(mask, cost, moves, cost_max)
        graph = coo_matrix((val.astype(np.float64), (dst, src)), shape=(n, n)).tocsr()  # (duplicate edges are summed by tocsr: see below)
        if len(src):
            # two moves of a state may lead to the same state (K = 1, K = 2): keep the cheaper, as the min does
            order = np.lexsort((val, src, dst))
            s2, d2, v2 = src[order], dst[order], val[order]
            first = np.ones(len(s2), bool)
            first[1:] = (s2[1:] != s2[:-1]) | (d2[1:] != d2[:-1])
            graph = coo_matrix((v2[first].astype(np.float64), (d2[first], s2[first])), shape=(n, n)).tocsr()
        dist = dijkstra(graph, directed=True, indices=sources, min_only=True)
        reached = np.isfinite(dist)
        D[reached] = dist[reached].astype(np.int64)
    return D.reshape(K, rows, cols)


# ---------------------------------------------------------------- next, best, counts, paths from the final D

def next_of(D, mask, cost, moves, cost_max):
    """d_next from a final (unbounded or masked) D: AT_GOAL where D == 0 (every move costs >= 1: the goal states alone), -1 where D is NONE,
    else the smallest slot whose admissible move attains D.  Whole planes at a time, the slots from the last to the first"""
    moves = np.asarray(moves)
    K, rows, cols = D.shape
    adm = admissible_of(mask, K)
    w = weights_of(cost, (rows, cols), cost_max)
    nxt = np.full(D.shape, -1, np.int64)
    for k in range(K):
        for m in reversed(range(MAX_MOVES)):
            da, db, k2, s = moves[k, m].tolist()
            if not s:
                continue
            ok = adm[k] & shifted(adm[k2], da, db, False)
            attains = ok & (shifted(D[k2], da, db, NONE) + s * shifted(w, da, db, 0) == D[k])
            nxt[k] = np.where(attains, m, nxt[k])
    reached = D != NONE
    assert (nxt[reached & (D != 0)] >= 0).all(), "D is no fixed point"
    nxt = np.where(D == 0, AT_GOAL, nxt)
    return np.where(reached, nxt, -1)


def path_from(start, D, nxt, moves, order):
    """the (cell, heading) pairs of the path from start = (linear index in `order` or -1, heading): [] for -1 or an unreached state"""
    K, rows, cols = D.shape
    cell, k = int(start[0]), int(start[1])
    if cell < 0:
        return []
    r, c = cell_of(cell, rows, cols, order)
    if D[k, r, c] == NONE:
        return []
    path = [(cell, k)]
    while D[k, r, c] != 0:
        da, db, k2, s = np.asarray(moves)[k, int(nxt[k, r, c])].tolist()
        assert s and len(path) <= K * rows * cols
        r, c, k = r + da, c + db, k2
        path.append((linear(r, c, rows, cols, order), k))
    return path


def expected_headings(mask, goals, cost, moves, goal_headings=ANY, cost_max=252, max_cost=0, order="row", start=None, max_len=0, sentinel=0,
                      search=cost_to_go):
    """the definition for one map: mask, goals, cost logical [rows, cols] (cost may be None), moves [K, 8, 4].  Returns dict(dist, next: int32
    [K, rows, cols], logical; best, best_heading: int32 [rows, cols]; counts: int32 [3] goal, reached, admissible states; path_len: int;
    path: int32 [max_len, 2], `sentinel` where the call writes nothing)"""
    moves = np.asarray(moves)
    K = moves.shape[0]
    rows, cols = np.asarray(goals).shape
    assert moves_ok(moves, K) and within_limit(rows, cols, K, moves, cost_max)
    D = search(mask, goals, cost, moves, goal_headings, cost_max)
    assert D.max() <= NONE
    if max_cost > 0:
        D = np.where(D > max_cost, NONE, D)
    nxt = next_of(D, mask, cost, moves, cost_max)
    best = D.min(axis=0)
    out = {"dist": D.astype(np.int32), "next": nxt.astype(np.int32), "best": best.astype(np.int32),
           "best_heading": np.where(best == NONE, -1, D.argmin(axis=0)).astype(np.int32),
           "counts": np.array([int((D == 0).sum()), int((D != NONE).sum()), int(admissible_of(mask, K).sum())], np.int32)}
    if start is not None:
        path = path_from(start, D, nxt, moves, order)
        rowbuf = np.full((max_len, 2), sentinel, np.int32)
        if path:
            rowbuf[:min(len(path), max_len)] = np.array(path[:max_len], np.int32)
        out["path"], out["path_len"], out["whole_path"] = rowbuf, len(path), path
    return out


# ---------------------------------------------------------------- scenes shared by the CPU and the GPU tests: (mask, goals, cost, start)

def random_scene(side, K, seed, density=0.25, n_goals=3):
    """a random heading mask: `density` of the cells admit no heading, the others lose each heading with probability 0.2; bits above K are set
    at random; costs across and beyond [1, cost_max] and at the int32 ends; a few goal cells.  start: the last cell with an admissible heading"""
    rng = np.random.default_rng(seed)
    bits = (rng.random((K, side, side)) > 0.2) & (rng.random((side, side)) > density)[None]
    mask = np.zeros((side, side), np.int64)
    for k in range(K):
        mask |= bits[k].astype(np.int64) << k
    if K < 32:
        mask |= rng.integers(0, 1 << (32 - K), (side, side)) << K
    cost = rng.integers(-5, 40, (side, side)).astype(np.int32)
    cost[rng.random((side, side)) < 0.02] = -2 ** 31
    cost[rng.random((side, side)) < 0.02] = 2 ** 31 - 1
    goals = np.full((side, side), -1, np.int32)
    for _ in range(n_goals):
        goals[rng.integers(side), rng.integers(side)] = rng.integers(0, 9)
    some = np.argwhere(bits.any(axis=0))
    goals[tuple(some[len(some) // 2])] = 0
    r, c = some[-1]
    return mask.astype(np.uint32).view(np.int32), goals, cost, (int(r), int(c), int(np.flatnonzero(bits[:, r, c])[0]))


def corridor_mask(side, K, cells, headings=None):
    """a mask that admits `headings` (all K by default) on the listed cells and nothing elsewhere"""
    mask = np.zeros((side, side), np.int64)
    word = sum(1 << k for k in (range(K) if headings is None else headings))
    for r, c in cells:
        mask[r, c] = word
    return mask.astype(np.uint32).view(np.int32)


def dead_end(side, K=8):
    """an open room (rows 1 .. 7, every heading) and below it a dead-end lane one cell wide down column side / 2 that admits only the two
    headings along it, 0 (looking down the lane, +row) and K / 2 (looking back out).  The goal state is the far end of the lane at heading
    K / 2, opposite to the heading a vehicle enters with; the start is in the room above the lane, looking in.  Forward-only moves can
    drive in but never face back out, so no chain reaches the goal state; with reverse moves the vehicle turns in the room and backs in.
    Returns (mask, goals, cost, start, goal_headings)"""
    c0 = side // 2
    cells = [(r, c) for r in range(1, 8) for c in range(1, side - 1)]
    mask = corridor_mask(side, K, cells).view(np.uint32).astype(np.int64)
    for r in range(8, side - 1):
        mask[r, c0] = (1 << 0) | (1 << (K // 2))
    goals = np.full((side, side), -1, np.int32)
    goals[side - 2, c0] = 0
    return mask.astype(np.uint32).view(np.int32), goals, None, (3, c0, 0), 1 << (K // 2)


def l_bend(side):
    """K = 4 (0: +row, 1: +col, 2: -row, 3: -col), a vehicle that is its reference cell and the cell behind it, lanes one cell wide: leg A
    down column 2 from row 1 to the corner (b, 2), a stub two cells on below the corner, leg B from the corner along row b to the goal at
    its end (any heading).  A lane cell admits the two headings along it; the corner admits 0 and 2 and also 3 (tail in leg B) but not 1
    (the tail would stand in the wall).  Forwards the vehicle can only arrive in the corner looking down or at the wall: no chain leads
    into leg B.  With reverse moves it drives past the corner into the stub, backs round into the corner (now heading 3) and backs along
    leg B.  Returns (mask, goals, cost, start, goal_headings)"""
    b = side // 2
    mask = np.zeros((side, side), np.int64)
    for r in range(1, b + 3):
        mask[r, 2] = 0b0101
    for c in range(3, side - 1):
        mask[b, c] = 0b1010
    mask[b, 2] = 0b1101
    goals = np.full((side, side), -1, np.int32)
    goals[b, side - 2] = 0
    return mask.astype(np.uint32).view(np.int32), goals, None, (1, 2, 0), ANY


# the random scenes of the GPU tests, one per (side, K): tests/test_route_headings_cpu.py asserts on the CPU that each of them has at least 10
# goal states, at least 100 reached non-goal states whose move changes the heading, and at least 10 admissible states that are not reached
RANDOM_SIDES, RANDOM_HEADINGS = (20, 23, 37, 41, 67), (8, 16, 32)


def random_table(side, K):
    """the helper's table of the random scene (side, K): steps 1, 2 and 3, with and without reverse moves and turns in place across the set"""
    j = RANDOM_SIDES.index(side) + RANDOM_HEADINGS.index(K)
    return table(K, step=1 + j % 3, unit=10, turn=3, reverse_pct=(0, 150)[(j // 3 + side) % 2], spin=(0, 25)[(j + K // 8) % 2 if K > 8 else 0])


def random_case(side, K):
    """(mask, goals, cost, start, moves) of the random scene (side, K)"""
    return random_scene(side, K, 7000 + 10 * side + K, density=0.2, n_goals=6) + (random_table(side, K),)


def scene_classes(want, moves):
    """(goal states, reached non-goal states whose move changes the heading, admissible unreached states) of an expectation"""
    D, nxt, moves = want["dist"], want["next"], np.asarray(moves)
    turning = 0
    for k in range(moves.shape[0]):
        for m in range(MAX_MOVES):
            if moves[k, m, 3] and moves[k, m, 2] != k:
                turning += int(((nxt[k] == m) & (D[k] > 0) & (D[k] != NONE)).sum())
    return int(want["counts"][0]), turning, int(want["counts"][2] - want["counts"][1])
