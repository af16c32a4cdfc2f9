"""What gg_visibility_clouds is expected to give, in numpy alone and without the library (a helper, not a test): the state of every cell --
OCCUPIED where the obstacle grid is, else FREE where a return landed or the integer ray from the sensor cell to the cell of a return passed,
else UNKNOWN -- from the closed form of include/groundgrid_hip.h, the scenes the GPU tests run, and the occupancy and the hits of real clouds
from the CPU oracle.  tests/test_visibility_clouds_cpu.py holds the closed form against exact rational arithmetic."""
import numpy as np

from tests import clearance_ref

FREE, UNKNOWN, OCCUPIED = -1, 0, 1


def ray_cells(r0, c0, r1, c1, max_cells=0):
    """the cells the ray from the sensor cell (r0, c0) to the end cell (r1, c1) CROSSES, in order, as two int64 arrays: for k = 0 .. n - 1
    (and only k < max_cells when that is > 0), n = max(|dr|, |dc|), the cell (r0 + sgn(dr) * ((2 k |dr| + n) // (2 n)), likewise for c)"""
    dr, dc = int(r1) - int(r0), int(c1) - int(c0)
    n = max(abs(dr), abs(dc))
    steps = n if max_cells == 0 else min(n, int(max_cells))
    k = np.arange(steps, dtype=np.int64)
    if n == 0:
        return k, k.copy()
    sr, sc = (dr > 0) - (dr < 0), (dc > 0) - (dc < 0)
    return r0 + sr * ((2 * k * abs(dr) + n) // (2 * n)), c0 + sc * ((2 * k * abs(dc) + n) // (2 * n))


def expected_visibility(occupied, hit, origin_cell, max_cells=0, order="row"):
    """occupied, hit: bool [rows, cols]; origin_cell: (r0, c0) or None (the sensor is in no cell: no ray).  Returns (state int32 laid out as
    the library lays the plane out -- [rows, cols] for "row", [cols, rows] for "col" --, counts int32 [3]: free, unknown, occupied)"""
    occupied, hit = np.asarray(occupied, dtype=bool), np.asarray(hit, dtype=bool)
    assert occupied.shape == hit.shape and order in ("row", "col") and max_cells >= 0
    crossed = np.zeros_like(hit)
    if origin_cell is not None:
        r0, c0 = int(origin_cell[0]), int(origin_cell[1])
        assert 0 <= r0 < hit.shape[0] and 0 <= c0 < hit.shape[1]
        for r1, c1 in np.argwhere(hit):
            rr, cc = ray_cells(r0, c0, r1, c1, max_cells)
            crossed[rr, cc] = True
    state = np.where(occupied, OCCUPIED, np.where(hit | crossed, FREE, UNKNOWN)).astype(np.int32)
    counts = np.array([(state == FREE).sum(), (state == UNKNOWN).sum(), (state == OCCUPIED).sum()], dtype=np.int32)
    return clearance_ref.as_plane(state, order), counts


# ---------------------------------------------------------------- the scenes of the GPU tests

OUTSIDE, NOT_FINITE = "outside", "nan"   # sensors that are in no cell


def ring_cells(r0, c0, radius):
    """the cells whose centre is `radius` cells (rounded) from (r0, c0)"""
    rr, cc = np.mgrid[r0 - radius - 1: r0 + radius + 2, c0 - radius - 1: c0 + radius + 2]
    on = np.rint(np.hypot(rr - r0, cc - c0)).astype(np.int64) == radius
    return [(int(a), int(b)) for a, b in zip(rr[on], cc[on])]


def scenes(size=79):
    """name -> dict(sensor=(r, c) | OUTSIDE | NOT_FINITE, occupied=[cells with two non-ground returns], ground=[cells with one ground
    return], single=[cells with one non-ground return: a hit that min_points = 2 does not make occupied]), in a fixed order.  `size` >= 79."""
    assert size >= 79
    m, e = size // 2, size - 1
    rng = np.random.default_rng(7100)
    S = {}

    def add(name, sensor, occupied=(), ground=(), single=()):
        S[name] = dict(sensor=sensor, occupied=list(occupied), ground=list(ground), single=list(single))

    add("octants", (m, m), ground=[(m + a, m + b) for a, b in ((7, 3), (7, -3), (-7, 3), (-7, -3), (3, 7), (3, -7), (-3, 7), (-3, -7))])
    add("octants_far", (m, m), ground=[(m + 37, m + 11), (m - 37, m + 11)], single=[(m + 11, m - 37), (m - 11, m - 37), (m + 5, m + 38), (m - 38, m - 29)],
        occupied=[(m + 36, m - 17), (m - 13, m + 36)])
    add("axes_and_diagonals", (m, m), ground=[(m, e), (m, 0), (0, m), (e, m)], single=[(m + 30, m + 30), (m - 30, m - 30), (m - 30, m + 30), (m + 30, m - 30)])
    add("halves_rows", (m, m), ground=[(m + sa * 20, m + sb * 10) for sa in (1, -1) for sb in (1, -1)] + [(m + sa * 6, m + sb * 3) for sa in (1, -1) for sb in (1, -1)])
    add("halves_cols", (m, m), ground=[(m + sa * 10, m + sb * 20) for sa in (1, -1) for sb in (1, -1)] + [(m + sa, m + sb * 2) for sa in (1, -1) for sb in (1, -1)])
    add("end_is_sensor", (20, 20), ground=[(20, 20)])
    add("corner_00", (0, 0), ground=[(e, e), (0, e), (e, 0)], single=[(40, 13), (1, 1)])
    add("corner_rc", (e, e), ground=[(0, 0), (e, 0), (0, e)], occupied=[(17, 60)])
    add("border_top", (0, 30), ground=[(e, 31), (0, 0), (0, e), (50, 77)])
    add("border_left", (30, 0), ground=[(31, e), (0, 0), (e, 0), (77, 50)])
    add("border_bottom", (e, 50), single=[(0, 49), (e, 0), (e, e), (2, 3)])
    add("border_right", (50, e), single=[(49, 0), (0, e), (e, e), (3, 2)])
    add("sensor_outside", OUTSIDE, occupied=[(10, 10), (60, 20)], ground=[(30, 30), (5, 70)], single=[(70, 70)])
    add("sensor_not_finite", NOT_FINITE, occupied=[(11, 12)], ground=[(33, 34), (6, 71)], single=[(71, 70)])
    add("through_occupied", (m, m), occupied=[(m, m + 11), (m + 8, m + 8)], ground=[(m, m + 21), (m + 16, m + 16)])
    add("single_nonground", (m, m), single=[(10, 50)])
    ring = ring_cells(m, m, 20)
    kinds = rng.integers(0, 3, len(ring))
    add("ring", (m, m), occupied=[c for c, k in zip(ring, kinds) if k == 0], ground=[c for c, k in zip(ring, kinds) if k == 1], single=[c for c, k in zip(ring, kinds) if k == 2])
    cells = [(int(a), int(b)) for a, b in zip(*np.unravel_index(rng.choice(size * size, 600, replace=False), (size, size)))]
    add("random", (int(rng.integers(0, size)), int(rng.integers(0, size))), occupied=cells[:200], ground=cells[200:400], single=cells[400:])
    add("empty", (m, m))
    add("all_outside", (m, m))   # (the test gives it points, every one outside the map)
    return S


def scene_truth(scene, size=79):
    """(occupied, hit, origin_cell or None) of a scene under min_points = 2 and an open height band"""
    occupied, hit = np.zeros((size, size), bool), np.zeros((size, size), bool)
    for r, c in scene["occupied"]:
        occupied[r, c] = hit[r, c] = True
    for r, c in scene["ground"] + scene["single"]:
        hit[r, c] = True
    sensor = scene["sensor"]
    return occupied, hit, None if sensor in (OUTSIDE, NOT_FINITE) else sensor


# ---------------------------------------------------------------- real clouds, through the CPU oracle

def cloud_truth(ref, cloud_map, labels, origin_xy, min_points=1, lo=-np.inf, hi=np.inf, ground=None):
    """(occupied, hit, origin_cell or None) of one cloud from the oracle: occupied as tests/test_cluster_clouds_gpu.expectation has it
    (ref's position and `ground` layer as they stand, or the constant `ground` of a fresh map), hit where OracleMap.get_index puts a point of
    label 49 or 99, the sensor cell by the same get_index on the float32 origin"""
    from tests.test_cluster_clouds_gpu import expectation

    n = len(cloud_map)
    labels = np.asarray(labels)[:n]
    occupied = expectation(ref, cloud_map, labels, min_points, lo, hi, 8, "row", ground=ground)[0] >= 0
    hit = np.zeros((ref.rows, ref.cols), bool)
    for p in np.nonzero((labels == 49) | (labels == 99))[0]:
        inside, r, c = ref.get_index(float(cloud_map["x"][p]), float(cloud_map["y"][p]))
        if inside and 0 <= r < ref.rows and 0 <= c < ref.cols:
            hit[r, c] = True
    ox, oy = float(np.float32(origin_xy[0])), float(np.float32(origin_xy[1]))
    origin = None
    if np.isfinite(ox) and np.isfinite(oy):
        inside, r, c = ref.get_index(ox, oy)
        if inside and 0 <= r < ref.rows and 0 <= c < ref.cols:
            origin = (int(r), int(c))
    assert not (occupied & ~hit).any()  # (a participating point is a return)
    return occupied, hit, origin
