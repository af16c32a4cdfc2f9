"""What gg_match_planes must write, restated in numpy from the text of include/groundgrid_hip.h alone: the rotated cell of every scan cell, the
score of one candidate (k, dy, dx) at a time by one integer gather, and the best candidate by an explicit lexicographic sort of all of them.
Every array here is LOGICAL, [rows, cols] indexed (row, col); `lay` puts one where `order` puts it in memory.  The arithmetic runs in int64
and is checked to fit an int32, so an overflow of the code under test cannot be shared.  tests/test_match_planes_cpu.py holds this file
against a restatement that shares no code with it (a count plane correlated with the padded field)."""
import numpy as np

UNIT = 16384
MAX_WINDOW, MAX_ROTATIONS, MAX_SIDE = 32, 64, 32768
LIMIT = (1 << 31) - 1
IDENTITY = np.array([[UNIT, 0]], np.int32)
DEFAULTS = dict(window=8, field_max=32)  # those of GroundSegmentation.match_planes


def lay(a, order):
    """a logical [rows, cols] array as the plane of `order`: [rows, cols] row-major, [cols, rows] column-major"""
    return np.ascontiguousarray(a if order == "row" else a.T)


def accepts(field_max, rows, cols):
    """the overflow limit of the header: what gg_match_planes accepts"""
    return field_max >= 1 and field_max * rows * cols <= LIMIT


def rnd(v):
    """(|v| + 8192) >> 14 with the sign of v: round half away from zero"""
    v = np.asarray(v, np.int64)
    return np.sign(v) * ((np.abs(v) + 8192) >> 14)


def rotated_cells(scan, pivot, pair):
    """(r', c') of every scan cell (word > 0), as two int64 arrays; duplicates stay"""
    r, c = np.nonzero(np.asarray(scan) > 0)
    pr, pc = int(pivot[0]), int(pivot[1])
    cq, sq = int(pair[0]), int(pair[1])
    dr, dc = r.astype(np.int64) - pr, c.astype(np.int64) - pc
    a, b = cq * dr - sq * dc, sq * dr + cq * dc
    assert np.abs(a).max(initial=0) < (1 << 31) and np.abs(b).max(initial=0) < (1 << 31)
    return pr + rnd(a), pc + rnd(b)


def score_of(field, field_max, rr, cc):
    """the sum of f over the cells (rr[i], cc[i]): f = min(max(word, 0), field_max) inside the map, 0 outside"""
    rows, cols = field.shape
    inside = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
    words = np.asarray(field)[rr[inside], cc[inside]].astype(np.int64)
    return int(np.clip(words, 0, field_max).sum())


def expected_match(scan, field, *, shift=None, pivot=None, rotations=None, window=8, field_max=32):
    """the contract for one map.  scan, field: [rows, cols] (any int32 words); shift (s0, s1) or None; pivot (row, col) or None;
    rotations [K, 2] or None.  Returns dict(best: int32 [6], scores: int32 [K, 2 W + 1, 2 W + 1])"""
    scan, field = np.asarray(scan), np.asarray(field)
    rows, cols = scan.shape
    assert field.shape == (rows, cols) and rows <= MAX_SIDE and cols <= MAX_SIDE and accepts(field_max, rows, cols)
    rotations = IDENTITY if rotations is None else np.asarray(rotations).reshape(-1, 2)
    K, W = len(rotations), int(window)
    assert 1 <= K <= MAX_ROTATIONS and 0 <= W <= MAX_WINDOW and np.abs(rotations).max() <= UNIT
    s0, s1 = (0, 0) if shift is None else (int(shift[0]), int(shift[1]))
    s0, s1 = min(max(s0, -rows), rows), min(max(s1, -cols), cols)
    pivot = (rows // 2, cols // 2) if pivot is None else pivot
    assert 0 <= pivot[0] < rows and 0 <= pivot[1] < cols
    D = 2 * W + 1
    scores = np.zeros((K, D, D), np.int64)
    n_cells = 0
    for k in range(K):
        rr, cc = rotated_cells(scan, pivot, rotations[k])
        n_cells = len(rr)
        for dy in range(-W, W + 1):
            for dx in range(-W, W + 1):
                scores[k, dy + W, dx + W] = score_of(field, field_max, rr + s0 + dy, cc + s1 + dx)
    assert scores.max(initial=0) <= LIMIT
    # every candidate as (-S, dy^2 + dx^2, k, dy, dx), sorted: the first one is the answer
    every = sorted((-int(scores[k, dy + W, dx + W]), dy * dy + dx * dx, k, dy, dx) for k in range(K) for dy in range(-W, W + 1) for dx in range(-W, W + 1))
    neg, _, k, dy, dx = every[0]
    ties = sum(1 for e in every if e[0] == neg)
    return dict(best=np.array([k, dy, dx, -neg, n_cells, ties], np.int32), scores=scores.astype(np.int32))


def rotation_table(angles_rad):
    """(round_half_away(16384 cos), round_half_away(16384 sin)) per angle, in float64 -- without numpy's rounding functions"""
    import math

    def half_away(v):
        return int(math.copysign(math.floor(abs(v) + 0.5), v))

    return np.array([[half_away(UNIT * math.cos(float(a))), half_away(UNIT * math.sin(float(a)))] for a in angles_rad], np.int32).reshape(-1, 2)
