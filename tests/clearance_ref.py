"""What gg_clearance_clouds is expected to give, in numpy alone and without the library (a helper, not a test): the exact squared Euclidean
distance of every cell to the nearest occupied cell, which cell that is, and the distance in metres as its float32 bits -- by brute force over
the occupied cells in ascending (row, col), the first minimum taken: that IS the tie rule (smallest row, then smallest column).  And the
occupancy patterns the tests run: those of tests/cluster_ref.py and the ones where equal distances decide.
tests/test_clearance_clouds_cpu.py holds expected_clearance against scipy.ndimage.distance_transform_edt."""
import numpy as np

from tests import cluster_ref

NONE = 0x7FFFFFFF       # GG_CLEARANCE_NONE
INF_BITS = 0x7F800000   # +inf as float32 bits


def expected_clearance(occupied, max_cells=0, order="row", res=0.33):
    """occupied: bool [rows, cols].  Returns (dist2 int32 [rows, cols], nearest int32 [rows, cols] -- the linear index in `order` of the
    nearest occupied cell, -1 without one --, distance uint32 [rows, cols] -- the bits of np.sqrt(np.float32(dist2)) * np.float32(res),
    +inf without one --, n_occupied).  max_cells = R > 0: a cell with dist2 > R * R has no obstacle."""
    occupied = np.asarray(occupied, dtype=bool)
    rows, cols = occupied.shape
    assert order in ("row", "col") and max_cells >= 0
    rr, cc = np.mgrid[0:rows, 0:cols].astype(np.int64)
    best = np.full((rows, cols), NONE, dtype=np.int64)
    near_r = np.full((rows, cols), -1, dtype=np.int64)
    near_c = np.full((rows, cols), -1, dtype=np.int64)
    cells = np.argwhere(occupied)  # (ascending (row, col))
    for r, c in cells:
        d2 = (rr - r) ** 2 + (cc - c) ** 2
        closer = d2 < best  # (strictly: the first minimum stays)
        best[closer] = d2[closer]
        near_r[closer], near_c[closer] = r, c
    if max_cells > 0:
        far = best > max_cells * max_cells
        best[far], near_r[far], near_c[far] = NONE, -1, -1
    none = best == NONE
    nearest = np.where(none, -1, cluster_ref.linear_index(near_r, near_c, rows, cols, order)).astype(np.int32)
    with np.errstate(invalid="ignore"):
        metres = (np.sqrt(np.where(none, 0, best).astype(np.float32)) * np.float32(res)).astype(np.float32)
    distance = np.where(none, np.uint32(INF_BITS), metres.view(np.uint32)).astype(np.uint32)
    return best.astype(np.int32), nearest, distance, int(len(cells))


def as_plane(grid, order):
    """a [rows, cols] array as the library lays the plane out: itself ("row") or its transpose ("col", [cols, rows])"""
    return np.ascontiguousarray(grid if order == "row" else grid.T)


def tie_patterns(rows=79, cols=79):
    """name -> bool [rows, cols]: the patterns in which several occupied cells are equally near"""
    assert rows >= 70 and cols >= 70
    P = {}
    corners = {"corner_00": (0, 0), "corner_0c": (0, cols - 1), "corner_r0": (rows - 1, 0), "corner_rc": (rows - 1, cols - 1)}
    for name, cell in corners.items():
        P[name] = np.zeros((rows, cols), dtype=bool)
        P[name][cell] = True
    P["four_corners"] = np.zeros((rows, cols), dtype=bool)  # (with odd sides the centre is a four-way tie)
    for cell in corners.values():
        P["four_corners"][cell] = True
    pairs = np.zeros((rows, cols), dtype=bool)  # a horizontal, a vertical and a diagonal pair, each with a cell exactly between them
    pairs[10, 20] = pairs[10, 26] = True        # (10, 23)
    pairs[30, 50] = pairs[38, 50] = True        # (34, 50)
    pairs[55, 10] = pairs[61, 16] = True        # (58, 13)
    P["pairs"] = pairs
    lines = np.zeros((rows, cols), dtype=bool)  # two full border lines
    lines[0, :] = lines[:, cols - 1] = True
    P["border_lines"] = lines
    return P


def patterns(rows=79, cols=79):
    """name -> bool [rows, cols], in a fixed order: cluster_ref.patterns, then tie_patterns"""
    P = dict(cluster_ref.patterns(rows, cols))
    P.update(tie_patterns(rows, cols))
    return P


def nearest_by_loop(occupied, r, c):
    """(dist2, r', c') of cell (r, c) by a plain loop of its own: the smallest distance, then the smallest row, then the smallest column;
    None without an occupied cell"""
    best = None
    for rr, cc in zip(*np.nonzero(occupied)):
        key = ((int(rr) - r) ** 2 + (int(cc) - c) ** 2, int(rr), int(cc))
        if best is None or key < best:
            best = key
    return best
