"""What gg_cluster_clouds is expected to give, in numpy and plain Python and without the library (a helper, not a test): the connected
components of a boolean occupancy array by a host union-find, numbered by ascending smallest linear cell index of `order`; the table of the
clusters and the per-point ids from the points' cells and heights; and the occupancy patterns the tests run.  The height keys are the
keys_of / floats_of idiom of tests/test_rasterize_clouds_gpu.py.  tests/test_cluster_clouds_cpu.py holds label_plane against
scipy.ndimage.label."""
import numpy as np

QUIET_NAN = 0x7FC00000
FIELDS = ["cells", "points", "row_min", "row_max", "col_min", "col_max", "height_max", "first_cell"]  # the eight words of a gg_cluster


def keys_of(h):
    """the order-preserving uint32 key of non-NaN float32 values: IEEE totalOrder as unsigned order"""
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def floats_of(keys):
    return np.where(keys >> 31, keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)


def linear_index(r, c, rows, cols, order):
    return r * cols + c if order == "row" else r + c * rows


def label_plane(occupied, connectivity=8, order="row"):
    """int32 [rows, cols]: -1 where `occupied` is False, else the id of the cell's connected component; the components are numbered
    0 .. K-1 in ascending order of their smallest linear cell index (order "row": r * cols + c, "col": r + c * rows)"""
    occupied = np.asarray(occupied, dtype=bool)
    rows, cols = occupied.shape
    assert connectivity in (4, 8) and order in ("row", "col")
    cells = [(int(r), int(c)) for r, c in zip(*np.nonzero(occupied))]
    parent = {rc: rc for rc in cells}

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    steps = [(-1, 0), (0, -1)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for r, c in cells:
        for dr, dc in steps:
            q = (r + dr, c + dc)
            if 0 <= q[0] < rows and 0 <= q[1] < cols and occupied[q]:
                a, b = find((r, c)), find(q)
                if a != b:
                    parent[a] = b
    smallest = {}
    for rc in cells:
        root = find(rc)
        smallest[root] = min(smallest.get(root, rows * cols), linear_index(rc[0], rc[1], rows, cols, order))
    ids = {root: k for k, root in enumerate(sorted(smallest, key=smallest.get))}
    plane = np.full((rows, cols), -1, dtype=np.int32)
    for rc in cells:
        plane[rc] = ids[find(rc)]
    return plane


def in_band(h, min_height, max_height):
    """!(h < min_height) && !(h > max_height), in float32: a NaN height is inside every band"""
    h = np.asarray(h, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return ~(h < np.float32(min_height)) & ~(h > np.float32(max_height))


def expected_clusters(rows, cols, point_row, point_col, h, participates, min_points=1, connectivity=8, order="row"):
    """point_row, point_col: the cell of every point (any value where it does not participate); h: float32 heights; participates: bool per
    point (label 99, inside the map, inside the band).  Returns (plane int32 [rows, cols], K, table uint32 [K, 8] -- the words of the K
    gg_cluster records, height_max as its bits --, point ids int32 [n])"""
    point_row, point_col = np.asarray(point_row, dtype=np.int64), np.asarray(point_col, dtype=np.int64)
    h, participates = np.asarray(h, dtype=np.float32), np.asarray(participates, dtype=bool)
    count = np.zeros((rows, cols), dtype=np.int64)
    np.add.at(count, (point_row[participates], point_col[participates]), 1)
    occupied = count >= min_points
    plane = label_plane(occupied, connectivity, order)
    K = int(plane.max()) + 1 if occupied.any() else 0
    ids = np.full(len(h), -1, dtype=np.int32)
    ids[participates] = plane[point_row[participates], point_col[participates]]
    table = np.zeros((K, 8), dtype=np.uint32)
    rr, cc = np.nonzero(occupied)
    of = plane[rr, cc]
    cells = np.bincount(of, minlength=K)
    lo_r, lo_c, first = np.full(K, rows), np.full(K, cols), np.full(K, rows * cols)
    hi_r, hi_c = np.full(K, -1), np.full(K, -1)
    np.minimum.at(lo_r, of, rr)
    np.maximum.at(hi_r, of, rr)
    np.minimum.at(lo_c, of, cc)
    np.maximum.at(hi_c, of, cc)
    np.minimum.at(first, of, linear_index(rr, cc, rows, cols, order))
    taken = ids >= 0
    points = np.bincount(ids[taken], minlength=K)
    top = np.zeros(K, dtype=np.uint32)
    real = taken & ~np.isnan(h)
    np.maximum.at(top, ids[real], keys_of(h[real]))
    for k, col in enumerate((cells, points, lo_r, hi_r, lo_c, hi_c)):
        table[:, k] = col.astype(np.int32).view(np.uint32)
    table[:, 6] = np.where(top == 0, np.uint32(QUIET_NAN), floats_of(top))
    table[:, 7] = first.astype(np.int32).view(np.uint32)
    return plane, K, table, ids


# ---------------------------------------------------------------- the occupancy patterns

def spiral(rows, cols):
    """a one-cell-wide path from the corner of the border inwards, a free lane between its turns: one cluster with the longest chains"""
    occ = np.zeros((rows, cols), dtype=bool)
    r, c, dr, dc = 0, 0, 0, 1
    occ[0, 0] = True

    def free(rr, cc):
        return 0 <= rr < rows and 0 <= cc < cols and not occ[rr, cc]

    def can_step(rr, cc, ddr, ddc):
        n1, n2 = (rr + ddr, cc + ddc), (rr + 2 * ddr, cc + 2 * ddc)
        beyond_ok = not (0 <= n2[0] < rows and 0 <= n2[1] < cols) or not occ[n2]
        return free(*n1) and beyond_ok

    for _ in range(rows * cols):  # (bounded: every step marks a new cell)
        if not can_step(r, c, dr, dc):
            dr, dc = dc, -dr  # turn right
            if not can_step(r, c, dr, dc):
                break
        r, c = r + dr, c + dc
        occ[r, c] = True
    return occ


def patterns(rows=79, cols=79):
    """name -> bool [rows, cols], in a fixed order"""
    assert rows >= 70 and cols >= 70
    P = {}
    P["empty"] = np.zeros((rows, cols), dtype=bool)
    P["full"] = np.ones((rows, cols), dtype=bool)
    rr, cc = np.mgrid[0:rows, 0:cols]
    P["checkerboard"] = (rr + cc) % 2 == 0
    P["spiral"] = spiral(rows, cols)
    comb = np.zeros((rows, cols), dtype=bool)  # teeth down the even columns, joined only along the last row
    comb[:, 0::2] = True
    comb[rows - 1, :] = True
    P["comb"] = comb
    P["comb_t"] = comb.T.copy() if rows == cols else comb[::-1, ::-1].copy()  # teeth along the rows, joined only along the last column
    u = np.zeros((rows, cols), dtype=bool)  # arms that meet only at the bottom
    u[5:66, 10] = u[5:66, 60] = True
    u[65, 10:61] = True
    P["u"] = u
    w = np.zeros((rows, cols), dtype=bool)
    w[3:70, 8] = w[20:70, 30] = w[10:70, 52] = w[1:70, 71] = True
    w[69, 8:72] = True
    P["w"] = w
    blocks = np.zeros((rows, cols), dtype=bool)  # pairs of blocks that touch at one corner only, along either diagonal
    blocks[10:20, 10:20] = blocks[20:30, 20:30] = True
    blocks[40:50, 30:40] = blocks[50:60, 20:30] = True
    P["corner_blocks"] = blocks
    edge = np.zeros((rows, cols), dtype=bool)  # the four corners and runs along the four border lines
    edge[0, 0] = edge[0, cols - 1] = edge[rows - 1, 0] = edge[rows - 1, cols - 1] = True
    edge[0, 5:31] = edge[rows - 1, 40:66] = True
    edge[10:51, 0] = edge[20:61, cols - 1] = True
    P["borders"] = edge
    trap = np.zeros((rows, cols), dtype=bool)  # consecutive linear indices across the border, in either order: no neighbours
    trap[30, cols - 1] = trap[31, 0] = True
    trap[rows - 1, 50] = trap[0, 51] = True
    P["trap"] = trap
    for density, seed in ((0.30, 5130), (0.45, 5145), (0.60, 5160)):
        P[f"random_{int(density * 100)}"] = np.random.default_rng(seed).random((rows, cols)) < density
    return P
