"""gg_score_rollouts in numpy and plain Python: a direct restatement of the contract of include/groundgrid_hip.h -- loops over maps,
rollouts and steps, Python integers (unbounded, so every "in 64 bits" of the contract holds trivially) -- and the scene builders of
tests/test_score_rollouts_cpu.py and tests/test_score_rollouts_gpu.py.  Planes are logical [rows, cols] arrays whatever the order; the
order only decides the linear index of end_cell (and how a test lays a plane out in memory)."""
import numpy as np

NONE = 0x7FFFFFFF
UNIT = 16384
RELATIVE, ABSOLUTE = 0, 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NO_START = (0, 0, 0, -1, -1, NONE, NONE, NONE)
FIELDS = ("steps", "len", "cost", "end_cell", "end_heading", "togo", "clear", "total")


def rha(v):
    """v / 16384 rounded half away from zero"""
    v = int(v)
    return -((-v + UNIT // 2) >> 14) if v < 0 else (v + UNIT // 2) >> 14


def linear(r, c, rows, cols, order):
    return r * cols + c if order == "row" else r + c * rows


def lay(plane, order):
    """a logical [rows, cols] plane as the words lie in memory in `order`"""
    return np.ascontiguousarray(plane if order == "row" else plane.T)


def pose(entry, start, K, frame, rotations):
    """(r16_t, c16_t, k_t) of a table entry (da, db, dk, s) from start (r16, c16, k0)"""
    da, db, dk = int(entry[0]), int(entry[1]), int(entry[2])
    r16, c16, k0 = (int(v) for v in start)
    if frame == ABSOLUTE:
        return da, db, dk % K
    cq, sq = int(rotations[k0][0]), int(rotations[k0][1])
    return r16 + rha(cq * da - sq * db), c16 + rha(sq * da + cq * db), (k0 + dk) % K


def score_one(table, start, K, frame, rotations, mask, cost, dist, clear, cost_max, reach, order):
    """the records [P, 8] and the best [4] of one map.  table: [T, P, 4] (step-major, as the call reads it); mask, cost, clear: logical
    [rows, cols] planes (cost, clear: or None); dist: [K, rows, cols] or None"""
    T, P = np.asarray(table).shape[:2]
    rows, cols = mask.shape
    records = np.empty((P, 8), np.int64)
    if int(start[0]) == -1:
        records[:] = NO_START
        return records, np.array([-1, NONE, 0, 0], np.int64)
    r16, c16, k0 = (int(v) for v in start)
    row0, col0 = r16 // 16, c16 // 16
    words, table = mask.view(np.uint32).tolist(), np.asarray(table).tolist()  # (Python integers from here on)
    cost, clear = None if cost is None else np.asarray(cost).tolist(), None if clear is None else np.asarray(clear).tolist()
    best_p, best_total, n_complete, n_scored = -1, NONE, 0, 0
    for p in range(P):
        length = T
        for t in range(T):
            if table[t][p][3] <= 0:
                length = t
                break
        steps, total_cost, low = 0, 0, NONE
        end_cell, end_k = linear(row0, col0, rows, cols, order), k0
        for t in range(length):
            pr, pc, k = pose(table[t][p], start, K, frame, rotations)
            r, c = pr // 16, pc // 16  # (Python floors towards minus infinity)
            if not (0 <= r < rows and 0 <= c < cols):
                break
            if reach > 0 and (abs(r - row0) > reach or abs(c - col0) > reach):
                break
            if not (words[r][c] >> k) & 1:
                break
            w = 1 if cost is None else min(max(cost[r][c], 1), cost_max)
            total_cost += min(table[t][p][3], 32767) * w
            if clear is not None:
                low = min(low, clear[r][c])
            end_cell, end_k = linear(r, c, rows, cols, order), k
            steps += 1
        complete = steps == length
        togo = NONE
        if complete:
            r, c = (end_cell // cols, end_cell % cols) if order == "row" else (end_cell % rows, end_cell // rows)
            togo = 0 if dist is None else int(dist[end_k, r, c])
        if steps == 0:
            low = NONE
        total = min(total_cost + togo, NONE - 1) if complete and togo != NONE and togo >= 0 else NONE
        records[p] = (steps, length, total_cost, end_cell, end_k, togo, low, total)
        n_complete += complete
        if total != NONE:
            n_scored += 1
            if total < best_total:  # (strictly: among equals the smallest p stays)
                best_p, best_total = p, total
    return records, np.array([best_p, best_total, n_complete, n_scored], np.int64)


def expected_rollouts(tables, starts, K, frame, rotations, masks, costs=None, dists=None, clears=None, cost_max=252, reach=0, order="row"):
    """dict(records int32 [n, P, 8], best int32 [n, 4]).  tables: [T, P, 4] shared or [n, T, P, 4]; starts [n, 3]; masks [n, rows, cols]
    logical planes; costs, clears: the same or None; dists: [n, K, rows, cols] or None"""
    tables, starts = np.asarray(tables), np.asarray(starts)
    n = len(masks)
    recs, bests = [], []
    for i in range(n):
        table = tables if tables.ndim == 3 else tables[i]
        r, b = score_one(table, starts[i], K, frame, rotations, np.asarray(masks[i]), None if costs is None else costs[i],
                         None if dists is None else dists[i], None if clears is None else clears[i], cost_max, reach, order)
        recs.append(r)
        bests.append(b)
    records, best = np.stack(recs), np.stack(bests)
    assert records.min() >= I32_MIN and records.max() <= I32_MAX
    return {"records": records.astype(np.int32), "best": best.astype(np.int32)}


# ---------------------------------------------------------------- scenes

def rotations_of(K):
    """K headings evenly round the circle, the Q14 pairs rounded half away from zero (api.rotation_table's arithmetic)"""
    a = 2.0 * np.pi * np.arange(K) / K
    v = np.stack([np.cos(a), np.sin(a)], axis=1) * float(UNIT)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)


def random_planes(side, K, seed, n=1, blocked=0.04):
    """(masks, costs, clears, dists) of n maps, logical planes: a mask whose cells lack random headings (and carry random bits above K), a
    cost plane with words below 1 and above any cost_max, a clearance plane with negative words, a D volume with GG_ROUTE_NONE and
    negative words here and there"""
    rng = np.random.default_rng([side, K, seed])
    bits = rng.integers(0, 1 << 32, (n, side, side), dtype=np.uint64)
    dense = rng.random((n, side, side)) < 0.93
    bits = np.where(dense, bits | ((1 << K) - 1), bits)
    bits = np.where(rng.random((n, side, side)) < blocked, bits & ~np.uint64((1 << K) - 1), bits)
    masks = bits.astype(np.uint32).view(np.int32)
    costs = rng.integers(-3, 400, (n, side, side)).astype(np.int32)
    clears = rng.integers(-2, 2000, (n, side, side)).astype(np.int32)
    dists = rng.integers(0, 100000, (n, K, side, side)).astype(np.int32)
    dists[rng.random(dists.shape) < 0.1] = NONE
    dists[rng.random(dists.shape) < 0.02] = -5
    return masks, costs, clears, dists


def mixed_table(P, T, K, side, seed, frame, n=None):
    """[T, P, 4] (n None) or [n, T, P, 4]: rollouts that wander a few cells per step from the middle of the map, so that some stay inside
    for all T steps, some leave it on each side and some cross any reach; every seventh ends early at a random step (s == 0 or negative),
    every eleventh is empty (s == 0 at t = 0); dk runs negative and beyond K"""
    rng = np.random.default_rng([P, T, K, side, seed, frame])
    shape = (T, P) if n is None else (n, T, P)
    heading = rng.integers(0, 4, shape[:-2] + (1, P))            # a side the rollout drifts to
    drift = rng.integers(0, 3, shape[:-2] + (1, P)) * 16 * max(1, side // (2 * T) + 1)
    t = np.arange(1, T + 1).reshape((T, 1))
    jitter = rng.integers(-24, 25, shape + (2,))
    along = drift * t
    da = np.where(heading == 0, along, np.where(heading == 1, -along, 0)) + jitter[..., 0]
    db = np.where(heading == 2, along, np.where(heading == 3, -along, 0)) + jitter[..., 1]
    if frame == ABSOLUTE:
        da, db = da + 16 * (side // 2) + 8, db + 16 * (side // 2) + 8
    dk = rng.integers(-3 * K - 1, 3 * K + 2, shape)
    s = rng.integers(1, 40, shape)
    s[rng.random(shape) < 0.01] = 40000  # (above 32767: clamped)
    p = np.arange(P)
    cut = rng.integers(0, T, shape[:-2] + (P,))
    ends = (t - 1 == cut[..., None, :]) & (p % 7 == 3)
    s = np.where(ends, np.where(p % 2 == 0, 0, -7), s)
    s[..., 0, :] = np.where(p % 11 == 5, 0, s[..., 0, :])
    return np.stack([da, db, dk, s], axis=-1).astype(np.int32)


def garbage_table(P, T, seed, n=None):
    """extreme words everywhere: every field draws from INT32_MIN, INT32_MAX, their neighbours, 0, +-1 and random words, s mostly positive"""
    rng = np.random.default_rng([P, T, seed, 99])
    shape = ((T, P) if n is None else (n, T, P)) + (4,)
    pool = np.array([I32_MIN, I32_MIN + 1, I32_MAX, I32_MAX - 1, 0, 1, -1, 16, -16, 1 << 30, -(1 << 30), 32767, 32768, 65536], np.int64)
    words = np.where(rng.random(shape) < 0.5, pool[rng.integers(0, len(pool), shape)], rng.integers(I32_MIN, I32_MAX + 1, shape))
    s = words[..., 3]
    words[..., 3] = np.where((s <= 0) & (rng.random(s.shape) < 0.8), I32_MAX, s)
    near = rng.random(shape[:-1]) < 0.3  # some poses near the map, so that a few steps are admissible before the garbage
    words[..., 0] = np.where(near, rng.integers(-40, 400, shape[:-1]), words[..., 0])
    words[..., 1] = np.where(near, rng.integers(-40, 400, shape[:-1]), words[..., 1])
    return words.astype(np.int32)


def sub_cell_starts(n, side, K, seed):
    """starts [n, 3] whose sixteenths run through 0, 8 and 15, near the middle of the map"""
    rng = np.random.default_rng([n, side, K, seed, 5])
    sub = np.array([0, 8, 15])
    cell = side // 2 + rng.integers(-2, 3, (n, 2))
    out = np.empty((n, 3), np.int32)
    out[:, 0] = 16 * cell[:, 0] + sub[np.arange(n) % 3]
    out[:, 1] = 16 * cell[:, 1] + sub[(np.arange(n) + 1) % 3]
    out[:, 2] = rng.integers(0, K, n)
    return out
