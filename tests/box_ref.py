"""The expectation of gg_box_clusters (include/groundgrid_hip.h) restated in numpy: int64 and uint64 arithmetic, vectorised over the
headings.  tests/test_box_clusters_cpu.py holds it, without the code under test, against a plain per-point loop, against answers fixed by
hand and against its invariants; tests/test_box_clusters_gpu.py holds the device against it on bits."""
import numpy as np

BOX_UNIT = 16
Q14 = 16384
MAX_HEADINGS, MAX_CLUSTERS = 32, 4096
AREA, EDGE = 0, 1
FIELDS = ("heading", "points", "a_min", "a_max", "b_min", "b_max", "cost_lo", "cost_hi")
BOX_DTYPE = np.dtype([(k, "<i4") for k in FIELDS])
NO_COST = np.uint64(0xFFFFFFFFFFFFFFFF)


def rotation_table(angles_rad):
    """(cq, sq) = (16384 cos, 16384 sin) rounded half away from zero, int32 [K, 2] (what api.rotation_table makes, restated)"""
    a = np.atleast_1d(np.asarray(angles_rad, dtype=np.float64))
    v = np.stack([np.cos(a), np.sin(a)], axis=1) * float(Q14)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)


def quantise(px, py, position, resolution):
    """(ux, uy) int64: floor(((double)p - pos) * s) with s = 16.0 / resolution in double; NaN and infinite coordinates give 0 (they never
    participate: the caller's `inside` refuses them)"""
    s = np.float64(BOX_UNIT) / np.float64(resolution)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((np.asarray(px, dtype=np.float32).astype(np.float64) - np.float64(position[0])) * s)
        fy = np.floor((np.asarray(py, dtype=np.float32).astype(np.float64) - np.float64(position[1])) * s)
    ok = np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2.0 ** 31) & (np.abs(fy) < 2.0 ** 31)
    return np.where(ok, fx, 0.0).astype(np.int64), np.where(ok, fy, 0.0).astype(np.int64)


def inside_map(px, py, position, resolution, rows, cols):
    """grid_map's checkIfPositionWithinMap and getIndexFromPosition on float32 points in double, as a boolean per point: the inside test of
    the path.  (The GPU tests take the CPU oracle's own answer instead.)"""
    res = np.float64(resolution)
    l0, l1 = np.float64(rows) * res, np.float64(cols) * res
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = np.asarray(px, dtype=np.float32).astype(np.float64), np.asarray(py, dtype=np.float32).astype(np.float64)
        tx, ty = -((x - position[0]) - 0.5 * l0), -((y - position[1]) - 0.5 * l1)
        inside = (tx >= 0.0) & (ty >= 0.0) & (tx < l0) & (ty < l1)
        r = np.trunc(-(((x - 0.5 * l0) - position[0]) / res))
        c = np.trunc(-(((y - 0.5 * l1) - position[1]) / res))
        return inside & (r >= 0) & (c >= 0) & (r < rows) & (c < cols)


def projections(ux, uy, rotations):
    """a, b int64 [points, K]"""
    rot = np.asarray(rotations, dtype=np.int64).reshape(-1, 2)
    cq, sq = rot[:, 0][None, :], rot[:, 1][None, :]
    ux, uy = np.asarray(ux, dtype=np.int64)[:, None], np.asarray(uy, dtype=np.int64)[:, None]
    return ux * cq + uy * sq, uy * cq - ux * sq


def expected_boxes(px, py, ids, n_clusters, position, resolution, rotations, criterion, max_clusters, inside):
    """One cloud.  px, py: the map-frame points (float32) of the cloud's n_points points; ids: their d_point_cluster words; n_clusters: the
    cloud's d_n_clusters word; inside: bool per point, the path's inside test.  Returns (M_i, records int32 [M_i, 8], costs uint64
    [M_i, K]): what the call writes; nothing behind M_i is."""
    rot = np.asarray(rotations, dtype=np.int64).reshape(-1, 2)
    K = rot.shape[0]
    assert 1 <= K <= MAX_HEADINGS and 1 <= max_clusters <= MAX_CLUSTERS and criterion in (AREA, EDGE)
    Mi = min(max(int(n_clusters), 0), int(max_clusters))
    ids = np.asarray(ids, dtype=np.int64)
    part = np.asarray(inside, dtype=bool) & (ids >= 0) & (ids < Mi)
    ux, uy = quantise(px, py, position, resolution)
    a, b = projections(ux, uy, rot)
    assert np.abs(a[part]).max(initial=0) < 2 ** 31 and np.abs(b[part]).max(initial=0) < 2 ** 31
    records, costs = np.zeros((Mi, 8), dtype=np.int32), np.full((Mi, K), NO_COST, dtype=np.uint64)
    records[:, 0] = -1
    for c in np.unique(ids[part]):
        sel = part & (ids == c)
        ac, bc = a[sel], b[sel]                                        # [m, K]
        lo_a, hi_a, lo_b, hi_b = ac.min(0), ac.max(0), bc.min(0), bc.max(0)
        if criterion == AREA:
            cost = (hi_a - lo_a).astype(np.uint64) * (hi_b - lo_b).astype(np.uint64)
        else:
            d = np.minimum(np.minimum(ac - lo_a, hi_a - ac), np.minimum(bc - lo_b, hi_b - bc))
            cost = d.sum(0).astype(np.uint64)
        k = int(np.argmin(cost))                                       # (the first among equals)
        records[c] = (k, int(sel.sum()), lo_a[k], hi_a[k], lo_b[k], hi_b[k], _i32(int(cost[k]) & 0xFFFFFFFF), _i32(int(cost[k]) >> 32))
        costs[c] = cost
    return Mi, records, costs


def _i32(word):
    """the int32 with the bits of a uint32 word"""
    return word - (1 << 32) if word >= (1 << 31) else word


def expected_boxes_loop(px, py, ids, n_clusters, position, resolution, rotations, criterion, max_clusters, inside):
    """The same by a plain loop over points and headings in Python integers: the second formulation the vectorised one is held against"""
    import math

    rot = [(int(c), int(s)) for c, s in np.asarray(rotations).reshape(-1, 2)]
    K = len(rot)
    Mi = min(max(int(n_clusters), 0), int(max_clusters))
    s = 16.0 / float(resolution)
    members = {}
    for p in range(len(ids)):
        c = int(ids[p])
        if not (0 <= c < Mi) or not bool(inside[p]):
            continue
        ux = math.floor((float(np.float32(px[p])) - float(position[0])) * s)
        uy = math.floor((float(np.float32(py[p])) - float(position[1])) * s)
        members.setdefault(c, []).append((ux, uy))
    records, costs = np.zeros((Mi, 8), dtype=np.int32), np.full((Mi, K), NO_COST, dtype=np.uint64)
    records[:, 0] = -1
    for c, pts in members.items():
        best = None
        for k, (cq, sq) in enumerate(rot):
            pa = [ux * cq + uy * sq for ux, uy in pts]
            pb = [uy * cq - ux * sq for ux, uy in pts]
            lo_a, hi_a, lo_b, hi_b = min(pa), max(pa), min(pb), max(pb)
            if criterion == AREA:
                cost = (hi_a - lo_a) * (hi_b - lo_b)
            else:
                cost = sum(min(u - lo_a, hi_a - u, v - lo_b, hi_b - v) for u, v in zip(pa, pb))
            costs[c, k] = cost
            if best is None or cost < best[0]:
                best = (cost, k, lo_a, hi_a, lo_b, hi_b)
        cost, k, lo_a, hi_a, lo_b, hi_b = best
        records[c] = (k, len(pts), lo_a, hi_a, lo_b, hi_b, _i32(cost & 0xFFFFFFFF), _i32(cost >> 32))
    return Mi, records, costs


def metric_box(record, rotations, resolution, position=(0.0, 0.0)):
    """float64 (centre x, centre y, length, width, yaw) of one record, computed the long way: the four corners of the rectangle in units,
    turned back into the map frame one by one, half a unit added for the floor, and averaged"""
    import math

    k = int(record[0])
    cq, sq = (float(v) / Q14 for v in np.asarray(rotations).reshape(-1, 2)[k])
    unit = float(resolution) / BOX_UNIT
    corners = []
    for pa in (float(record[2]), float(record[3])):
        for pb in (float(record[4]), float(record[5])):
            ua, ub = pa / Q14, pb / Q14
            corners.append(((ua * cq - ub * sq + 0.5) * unit + position[0], (ua * sq + ub * cq + 0.5) * unit + position[1]))
    cx, cy = sum(p[0] for p in corners) / 4.0, sum(p[1] for p in corners) / 4.0
    return cx, cy, (float(record[3]) - float(record[2])) / Q14 * unit, (float(record[5]) - float(record[4])) / Q14 * unit, math.atan2(sq, cq)
