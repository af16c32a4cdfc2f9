"""gg_footprint_planes and gg_footprint_spans restated in numpy and plain Python integers from the text of include/groundgrid_hip.h alone: no
call into the library.  rect_spans is the span table of a rectangle (every cell of the box [-33, 33]^2 tested one by one);
expected_footprint is the definition for one map, computed by OR-ing shifted copies of the padded blocked plane."""
import math

import numpy as np

UNIT = 16384            # 1.0 of a rotation pair and of a rectangle word (Q14)
MAX_HEADINGS = 32
MAX_RADIUS = 32
BOX = MAX_RADIUS + 1    # gg_footprint_spans evaluates the test on [-BOX, BOX]^2
RECT_LIMIT = 1 << 30
EMPTY = (1, 0)          # how gg_footprint_spans stores an empty row
# the car of the issue: 4.7 m x 1.9 m on 0.33 m cells, the reference cell at the rear axle (ahead, behind, left, right in cells), the
# default pad of api.footprint_spans, 32 headings
CAR = dict(ahead=11.2, behind=3.0, left=2.9, right=2.9)
CAR_PAD = 0.7072
CAR_RADIUS = 14


def q14(v):
    """a length in cells as units of 1 / 16384 cell, rounded half away from zero"""
    m = math.floor(abs(float(v)) * UNIT + 0.5)
    return -m if v < 0 else m


def rotation_table(angles_rad):
    """plain-integer (cq, sq) pairs of the angles, each word rounded half away from zero (api.rotation_table)"""
    return [(q14(math.cos(a)), q14(math.sin(a))) for a in angles_rad]


def headings(K):
    """K evenly spaced headings, the first along the row axis"""
    return rotation_table([2.0 * math.pi * k / K for k in range(K)])


def rect_of(ahead, behind, left, right, pad=CAR_PAD):
    """(u_lo, u_hi, v_lo, v_hi) of gg_footprint_spans as api.footprint_spans makes it"""
    return (q14(-(behind + pad)), q14(ahead + pad), q14(-(right + pad)), q14(left + pad))


def rect_cells(pair, rect):
    """the member cells (a, b) of one heading on the box, by the membership test of the header"""
    cq, sq = int(pair[0]), int(pair[1])
    u_lo, u_hi, v_lo, v_hi = (int(w) for w in rect)
    cells = set()
    for a in range(-BOX, BOX + 1):
        for b in range(-BOX, BOX + 1):
            u, v = cq * a + sq * b, -sq * a + cq * b
            if u_lo <= u <= u_hi and v_lo <= v <= v_hi:
                cells.add((a, b))
    return cells


def needed_of(rotations, rect):
    """the largest Chebyshev norm of a member cell over all headings, -1 when there is none"""
    return max([max(abs(a), abs(b)) for pair in rotations for a, b in rect_cells(pair, rect)], default=-1)


def rect_spans(rotations, rect, radius):
    """the table [K][2 radius + 1][2] of a rectangle as nested lists of plain integers, or None when a member lies beyond `radius`"""
    if needed_of(rotations, rect) > radius:
        return None
    table = []
    for pair in rotations:
        cells = rect_cells(pair, rect)
        rows = []
        for a in range(-radius, radius + 1):
            bs = sorted(b for (aa, b) in cells if aa == a)
            assert bs == list(range(bs[0], bs[-1] + 1)) if bs else True  # row-convex by construction
            rows.append([bs[0], bs[-1]] if bs else list(EMPTY))
        table.append(rows)
    return table


def car_spans(K=32, radius=CAR_RADIUS):
    return np.array(rect_spans(headings(K), rect_of(**CAR), radius), np.int32)


def cells_of(spans, k):
    """F_k of a span table [K, 2 R + 1, 2] as a sorted list of (a, b)"""
    spans = np.asarray(spans)
    R = spans.shape[1] // 2
    return [(a, b) for a in range(-R, R + 1) for b in range(int(spans[k, a + R, 0]), int(spans[k, a + R, 1]) + 1)]


def is_convex(spans, k):
    """row-convex by the table's form; column-convex iff for every b the rows that hold it are consecutive"""
    by_col = {}
    for a, b in cells_of(spans, k):
        by_col.setdefault(b, []).append(a)
    return all(rows == list(range(rows[0], rows[-1] + 1)) for rows in by_col.values())


def valid_table(spans):
    """what gg_footprint_planes asks of a table: 1 <= K <= 32, 0 <= R <= 32, non-empty rows inside [-R, R], every heading column-convex"""
    spans = np.asarray(spans)
    if spans.ndim != 3 or spans.shape[2] != 2 or spans.shape[1] % 2 != 1:
        return False
    K, R = spans.shape[0], spans.shape[1] // 2
    if not (1 <= K <= MAX_HEADINGS and R <= MAX_RADIUS):
        return False
    lo, hi = spans[..., 0].astype(np.int64), spans[..., 1].astype(np.int64)
    full = lo <= hi
    if ((lo < -R) & full).any() or ((hi > R) & full).any():
        return False
    return all(is_convex(spans, k) for k in range(K))


def expected_footprint(blocked, spans, min_fit, outside_free):
    """the definition for one map: blocked a logical int32 [rows, cols] plane (blocked where the word is >= 0), spans int32 [K, 2 R + 1, 2].
    Returns dict(mask: uint32 [rows, cols]; fit: int32 [rows, cols]; counts: int32 [3]; p: the number of fitting headings per cell)"""
    blocked, spans = np.asarray(blocked), np.asarray(spans)
    assert valid_table(spans) and outside_free in (0, 1, False, True)
    rows, cols = blocked.shape
    K, R = spans.shape[0], spans.shape[1] // 2
    assert 1 <= min_fit <= K
    pad = np.full((rows + 2 * R, cols + 2 * R), not outside_free, bool)  # the outside rule
    pad[R: R + rows, R: R + cols] = blocked >= 0
    mask = np.zeros((rows, cols), np.uint32)
    for k in range(K):
        hit = np.zeros((rows, cols), bool)  # some cell of F_k laid at (r, c) is blocked
        for a, b in cells_of(spans, k):
            hit |= pad[R + a: R + a + rows, R + b: R + b + cols]  # cell (r + a, c + b)
        mask |= np.where(hit, 0, 1 << k).astype(np.uint32)
    p = np.zeros((rows, cols), np.int32)
    for k in range(K):
        p += ((mask >> np.uint32(k)) & np.uint32(1)).astype(np.int32)
    fit = np.where(p >= min_fit, -1, p).astype(np.int32)
    counts = np.array([int((p == K).sum()), int((p >= min_fit).sum()), int((p == 0).sum())], np.int32)
    return dict(mask=mask, fit=fit, counts=counts, p=p)


# ---------------------------------------------------------------- the scenes of the tests (shared, so that the CPU tests can hold what the GPU tests rely on)

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SCENES = ("random", "free", "full", "rim", "one", "extremes", "seams")
# the draw of the random scene by side: at side 67 most draws leave the car no cell where all 32 headings fit with the outside blocked; this
# one does (tests/test_footprint_planes_cpu.py asserts the three classes of every random scene)
RANDOM_SEED = {67: 8}
SEAMS = (31, 32, 63, 64, 95, 96)  # lines and columns on either side of every tile and word seam of a 128 x 128 plane


def scene(name, side):
    """the blocked plane of one map, logical int32 [side, side]: blocked where the word is >= 0"""
    rng = np.random.default_rng(2100 + 31 * side + SCENES.index(name))
    free = rng.integers(I32_MIN, 0, (side, side), dtype=np.int64)  # any negative word is free
    taken = rng.integers(0, 1 << 31, (side, side), dtype=np.int64)  # any word >= 0 is blocked
    if name == "random":  # (1 % blocked: at 5 % the car fits almost nowhere)
        is_blocked = np.random.default_rng(RANDOM_SEED.get(side, side)).random((side, side)) < 0.01
    elif name == "free":
        is_blocked = np.zeros((side, side), bool)
    elif name == "full":
        is_blocked = np.ones((side, side), bool)
    elif name == "rim":
        is_blocked = np.ones((side, side), bool)
        is_blocked[1:-1, 1:-1] = False
    elif name == "one":  # off-centre, so that a reflected or transposed answer differs
        is_blocked = np.zeros((side, side), bool)
        is_blocked[side // 2 - 2, side // 2 + 3] = True
    elif name == "extremes":  # the words next to the threshold and at both ends of the range
        return rng.choice(np.array([I32_MIN, -1, 0, I32_MAX], np.int64), (side, side), p=[0.49, 0.49, 0.01, 0.01]).astype(np.int32)
    elif name == "seams":  # single blocked cells on the seam lines and columns, where they exist, a few per seam
        is_blocked = np.zeros((side, side), bool)
        for j, s in enumerate(s for s in SEAMS if s < side):
            for i in range(3):
                is_blocked[s, (11 + 37 * i + 7 * j) % side] = True
                is_blocked[(5 + 41 * i + 13 * j) % side, s] = True
    return np.where(is_blocked, taken, free).astype(np.int32)
