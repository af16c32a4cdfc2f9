"""What the labelled-cloud calls (gg_split_clouds, gg_rasterize_clouds, gg_cluster_clouds, gg_clearance_clouds in cloud mode,
gg_visibility_clouds) are expected to give for one cloud, from the CPU oracle and numpy alone (a helper, not a test; importable without a
GPU).  `ref` is an oracle.OracleMap: its position and `ground` layer as they stand (or the constant `ground` of a fresh map), cloud_map the
points in the map frame, labels one byte per point of it.  expected_sets and expected_planes are the expectations of
tests/test_split_clouds_gpu.py and tests/test_rasterize_clouds_gpu.py, kept here so that tests/seq_model.py can use them too; point_cells
and the three functions behind it put tests/cluster_ref.py, clearance_ref.py and visibility_ref.py on top of the same cells and heights."""
import numpy as np

from groundgrid_amd import api
from tests import clearance_ref, cluster_ref, visibility_ref

QUIET_NAN = 0x7FC00000
SETS = ("ground", "nonground")
CODE = {"ground": 49, "nonground": 99}


def keys_of(h):
    """the order-preserving uint32 key of non-NaN float32 values: IEEE totalOrder as unsigned order"""
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def floats_of(keys):
    return np.where(keys >> 31, keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)


def expected_sets(ref, cloud_map, labels, ground=None):
    """{set: (source indices, packed records, heights)} of one cloud from the oracle: ref's position and `ground` layer as they stand (or the
    constant `ground` of a fresh map), cloud_map the points in the map frame, labels one byte per point of it"""
    layer = ref.layer("ground")
    out = {}
    for s in SETS:
        idx = np.nonzero(labels[: len(cloud_map)] == CODE[s])[0].astype(np.int32)
        h = np.empty(len(idx), dtype=np.float32)
        for k, p in enumerate(idx):
            inside, r, c = ref.get_index(float(cloud_map["x"][p]), float(cloud_map["y"][p]))
            if inside and 0 <= r < ref.rows and 0 <= c < ref.cols:
                h[k] = np.float32(cloud_map["z"][p]) - (layer[r, c] if ground is None else np.float32(ground))
            else:
                h[k : k + 1].view(np.uint32)[0] = QUIET_NAN
        out[s] = (idx, api.pack16(cloud_map[idx]), h)
    return out


def expected_planes(ref, cloud_map, labels, ground=None):
    """uint32 [6, rows, cols]: the bits of the six channels of one cloud in GG_RASTER_* order, from the oracle: ref's position and `ground`
    layer as they stand (or the constant `ground` of a fresh map), cloud_map the points in the map frame, labels one byte per point"""
    rows, cols = ref.rows, ref.cols
    layer = ref.layer("ground")
    out = np.empty((6, rows * cols), dtype=np.uint32)
    for s, code in enumerate((99, 49)):
        idx = np.nonzero(labels[: len(cloud_map)] == code)[0]
        cells, hs = [], []
        for p in idx:
            inside, r, c = ref.get_index(float(cloud_map["x"][p]), float(cloud_map["y"][p]))
            if inside and 0 <= r < rows and 0 <= c < cols:
                cells.append(r * cols + c)
                with np.errstate(invalid="ignore", over="ignore"):
                    hs.append(np.float32(cloud_map["z"][p]) - (layer[r, c] if ground is None else np.float32(ground)))
        cells, hs = np.array(cells, dtype=np.int64), np.array(hs, dtype=np.float32)
        count = np.zeros(rows * cols, dtype=np.uint32)
        np.add.at(count, cells, 1)
        ok = ~np.isnan(hs)
        hi, lo = np.zeros(rows * cols, dtype=np.uint32), np.full(rows * cols, 0xFFFFFFFF, dtype=np.uint32)
        np.maximum.at(hi, cells[ok], keys_of(hs[ok]))
        np.minimum.at(lo, cells[ok], keys_of(hs[ok]))
        out[3 * s] = count.astype(np.float32).view(np.uint32)
        out[3 * s + 1] = np.where(hi == 0, np.uint32(QUIET_NAN), floats_of(hi))
        out[3 * s + 2] = np.where(lo == 0xFFFFFFFF, np.uint32(QUIET_NAN), floats_of(lo))
    return out.reshape(6, rows, cols)


def point_cells(ref, cloud_map, labels, ground=None):
    """per point of the cloud: (inside bool, row int64, col int64, h float32) for the points whose label is 49 or 99 (inside = False and
    zeros for every other point): OracleMap.get_index under ref's position, h = np.float32(z) - ground[row, col]"""
    n = len(cloud_map)
    labels = np.asarray(labels)[:n]
    layer = ref.layer("ground")
    inside, pr, pc, h = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
    for p in np.nonzero((labels == 49) | (labels == 99))[0]:
        ok, r, c = ref.get_index(float(cloud_map["x"][p]), float(cloud_map["y"][p]))
        if ok and 0 <= r < ref.rows and 0 <= c < ref.cols:
            with np.errstate(invalid="ignore", over="ignore"):
                h[p] = np.float32(cloud_map["z"][p]) - (layer[r, c] if ground is None else np.float32(ground))
            inside[p], pr[p], pc[p] = True, r, c
    return inside, pr, pc, h


def expected_clusters(ref, cloud_map, labels, min_points=1, lo=-np.inf, hi=np.inf, conn=8, order="row", ground=None):
    """cluster_ref.expected_clusters of one cloud: (plane int32 [rows, cols], K, table uint32 [K, 8], point ids int32 [n])"""
    inside, pr, pc, h = point_cells(ref, cloud_map, labels, ground)
    part = inside & (np.asarray(labels)[: len(cloud_map)] == 99) & cluster_ref.in_band(h, lo, hi)
    return cluster_ref.expected_clusters(ref.rows, ref.cols, pr, pc, h, part, min_points, conn, order)


def occupied_cells(ref, cloud_map, labels, min_points=1, lo=-np.inf, hi=np.inf, ground=None, cells=None):
    """bool [rows, cols]: where gg_cluster_clouds with the same arguments writes d_cell_cluster >= 0"""
    inside, pr, pc, h = point_cells(ref, cloud_map, labels, ground) if cells is None else cells
    part = inside & (np.asarray(labels)[: len(cloud_map)] == 99) & cluster_ref.in_band(h, lo, hi)
    count = np.zeros((ref.rows, ref.cols), dtype=np.int64)
    np.add.at(count, (pr[part], pc[part]), 1)
    return count >= min_points


def expected_clearance_fast(occupied, max_cells=0, res=0.33):
    """(dist2 int32 [rows, cols], distance bits uint32 [rows, cols], n_occupied) as clearance_ref.expected_clearance gives them, from
    scipy.ndimage.distance_transform_edt(return_indices=True): the squared distance to the feature it names is the exact minimum whatever
    its tie rule (so `nearest` is not available here)"""
    from scipy import ndimage

    occupied = np.asarray(occupied, dtype=bool)
    rows, cols = occupied.shape
    if not occupied.any():
        best = np.full((rows, cols), clearance_ref.NONE, dtype=np.int64)
    else:
        ind = ndimage.distance_transform_edt(~occupied, return_distances=False, return_indices=True)
        rr, cc = np.mgrid[0:rows, 0:cols].astype(np.int64)
        best = (rr - ind[0]) ** 2 + (cc - ind[1]) ** 2
        if max_cells > 0:
            best[best > max_cells * max_cells] = clearance_ref.NONE
    none = best == clearance_ref.NONE
    metres = (np.sqrt(np.where(none, 0, best).astype(np.float32)) * np.float32(res)).astype(np.float32)
    distance = np.where(none, np.uint32(clearance_ref.INF_BITS), metres.view(np.uint32)).astype(np.uint32)
    return best.astype(np.int32), distance, int(occupied.sum())


def expected_visibility(ref, cloud_map, labels, origin_xy, min_points=1, lo=-np.inf, hi=np.inf, max_cells=0, order="row", ground=None):
    """visibility_ref.expected_visibility of one cloud: (state int32 plane as the library lays it out, counts int32 [3])"""
    cells = point_cells(ref, cloud_map, labels, ground)
    occupied = occupied_cells(ref, cloud_map, labels, min_points, lo, hi, cells=cells)
    inside, pr, pc, _ = cells
    hit = np.zeros((ref.rows, ref.cols), bool)
    hit[pr[inside], pc[inside]] = True
    ox, oy = float(np.float32(origin_xy[0])), float(np.float32(origin_xy[1]))
    origin = None
    if np.isfinite(ox) and np.isfinite(oy):
        ok, r, c = ref.get_index(ox, oy)
        if ok and 0 <= r < ref.rows and 0 <= c < ref.cols:
            origin = (int(r), int(c))
    return visibility_ref.expected_visibility(occupied, hit, origin, max_cells, order)
