"""gg_cluster_clouds (the connected components of the occupied cells of many clouds' obstacle grids: an id plane, a table of the clusters and
an id per point, in device memory, one call) on the device.  Expected values come from the CPU oracle, numpy and a plain host union-find
alone (tests/cluster_ref.py, itself held against scipy.ndimage.label by tests/test_cluster_clouds_cpu.py): OracleMap.filter_cloud gives the
labels and the `ground` layer afterwards, OracleMap.get_index the cell, np.float32(z) - ground[row, col] the height.  Every comparison is on
bits; there is no tolerance."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, kitti, synth  # noqa: E402
from groundgrid_amd._lib import LAYERS  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import cluster_ref  # noqa: E402
from tests.test_export_layers_gpu import SENTINEL, batch_points, fresh_count, same_bits, stride_of, warm_maps  # noqa: E402
from tests.test_split_clouds_gpu import GEOMETRY, PARAM_RING, lazy_count, masks_of, points_tensor, transform_of  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
SIGNED_SENTINEL = SENTINEL - (1 << 32) if SENTINEL >= (1 << 31) else SENTINEL
INF = math.inf


# ---------------------------------------------------------------- helpers

class Dest:
    """sentinel-filled destinations of one call: n planes plane_stride words apart, the per-point ids, the counts and the table"""

    def __init__(self, n, plane_stride, cloud_stride, max_clusters, slack=0):
        import torch

        def filled(words):
            return torch.full((max(words, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

        self.n, self.plane_stride, self.cloud_stride, self.max_clusters = n, plane_stride, cloud_stride, max_clusters
        self.planes, self.ids, self.counts, self.table = filled(n * plane_stride + slack), filled(n * cloud_stride), filled(n), filled(n * max_clusters * 8)

    def host(self):
        return dict(planes=self.planes.cpu().numpy().view(np.uint32), ids=self.ids.cpu().numpy().view(np.uint32).reshape(self.n, -1),
                    counts=self.counts.cpu().numpy().view(np.uint32), table=self.table.cpu().numpy().view(np.uint32).reshape(self.n, -1, 8))

    def all_sentinel(self):
        return all(bool((t == SIGNED_SENTINEL).all().item()) for t in (self.planes, self.ids, self.counts, self.table))


def raw_cluster(seg, n, slots, first_slot, fmt, points, stride, n_points, dest, labels=0, masks=0, transforms=None, min_points=1, lo=-INF, hi=INF,
                conn=8, order=ROW, stream=None, own=False, **over):
    """gg_cluster_clouds as the C ABI has it (device addresses as integers, 0 = null); returns the status.  `over`: cell, plane_stride, ids,
    counts, table, max_clusters in place of what `dest` gives"""
    import torch

    x = _lib.GGCloudClusters()
    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    npts = None if n_points is None else (C.c_int32 * max(len(n_points), 1))(*[int(v) for v in n_points])
    x.n, x.first_slot, x.slots, x.point_format = n, first_slot, sl, fmt
    x.d_points, x.cloud_stride, x.n_points = points or None, stride, npts
    tfs = None
    if transforms is not None:
        tfs = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(-1, 12))
        x.transforms = tfs.ctypes.data_as(C.POINTER(C.c_double))
    x.d_labels, x.d_label_masks = labels or None, masks or None
    x.min_points, x.min_height, x.max_height, x.connectivity, x.order = min_points, lo, hi, conn, order
    x.d_cell_cluster = over.get("cell", dest.planes.data_ptr()) or None
    x.plane_stride = over.get("plane_stride", dest.plane_stride)
    x.d_point_cluster = over.get("ids", dest.ids.data_ptr()) or None
    x.d_n_clusters = over.get("counts", dest.counts.data_ptr()) or None
    x.d_clusters = over.get("table", dest.table.data_ptr() if dest.max_clusters else 0) or None
    x.max_clusters = over.get("max_clusters", dest.max_clusters)
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_cluster_clouds(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def expectation(ref, cloud_map, labels, min_points=1, lo=-INF, hi=INF, conn=8, order="row", ground=None):
    """cluster_ref.expected_clusters of one cloud from the oracle: ref's position and `ground` layer as they stand (or the constant `ground`
    of a fresh map), cloud_map the points in the map frame, labels one byte per point"""
    n = len(cloud_map)
    layer = ref.layer("ground")
    pr, pc, h, part = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32), np.zeros(n, bool)
    for p in np.nonzero(labels[:n] == 99)[0]:
        inside, r, c = ref.get_index(float(cloud_map["x"][p]), float(cloud_map["y"][p]))
        if inside and 0 <= r < ref.rows and 0 <= c < ref.cols:
            with np.errstate(invalid="ignore", over="ignore"):
                h[p] = np.float32(cloud_map["z"][p]) - (layer[r, c] if ground is None else np.float32(ground))
            pr[p], pc[p], part[p] = r, c, True
    part &= cluster_ref.in_band(h, lo, hi)
    return cluster_ref.expected_clusters(ref.rows, ref.cols, pr, pc, h, part, min_points, conn, order)


def check_cloud(host, i, want, n_points, order, rows, cols, plane_stride, max_clusters, tag):
    """cloud i of a downloaded Dest against an expectation: the plane, the count, the records, the per-point ids, and nothing else written"""
    plane, K, table, ids = want
    at = i * plane_stride
    got = host["planes"][at: at + rows * cols].view(np.int32)
    got = got.reshape(rows, cols) if order == ROW else got.reshape((rows, cols), order="F")
    bad = int((got != plane).sum())
    assert bad == 0, f"{tag}: cloud {i}: {bad} cells of the id plane differ"
    assert np.all(host["planes"][at + rows * cols: at + plane_stride] == SENTINEL), f"{tag}: cloud {i}: the words behind the plane were written"
    assert int(host["counts"][i]) == K, f"{tag}: cloud {i}: n_clusters {int(host['counts'][i])} != {K}"
    if max_clusters:
        m = min(K, max_clusters)
        for k, name in enumerate(cluster_ref.FIELDS):
            bad = np.nonzero(host["table"][i, :m, k] != table[:m, k])[0]
            assert len(bad) == 0, f"{tag}: cloud {i}: {name} of {len(bad)} records differs, first {bad[0]}: {host['table'][i, bad[0], k]:#x} != {table[bad[0], k]:#x}"
        assert np.all(host["table"][i, m:] == SENTINEL), f"{tag}: cloud {i}: records behind min(K, max_clusters) were written"
    bad = int((host["ids"][i, :n_points].view(np.int32) != ids).sum())
    assert bad == 0, f"{tag}: cloud {i}: {bad} per-point ids differ"
    assert np.all(host["ids"][i, n_points:] == SENTINEL), f"{tag}: cloud {i}: ids behind n_points were written"


def cell_centres(ref, cells):
    """map-frame (x, y) float32 of the centres of cells [(row, col)] of an unmoved map; get_index is held to put every one where it is meant"""
    res, (lx, ly), (px, py) = ref.resolution, ref.length, ref.position
    rc = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    x = (px + 0.5 * lx - (rc[:, 0] + 0.5) * res).astype(np.float32)
    y = (py + 0.5 * ly - (rc[:, 1] + 0.5) * res).astype(np.float32)
    for k in range(len(rc)):
        assert ref.get_index(float(x[k]), float(y[k])) == (True, int(rc[k, 0]), int(rc[k, 1])), (rc[k], x[k], y[k])
    return x, y


def cloud_of(x, y, z):
    cloud = synth.empty_cloud(len(x))
    cloud["x"], cloud["y"], cloud["z"] = x, y, z
    return cloud


def small_chunk_context(n_slots, max_points, size=79):
    length, res = GEOMETRY[size]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GG_PW", "128")  # (read at gg_create: a cloud of 6241 points spans 49 chunks and 13 work-groups)
        seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=max_points)
    assert seg.debug_set_tuning("pw", 0) == 128
    assert seg.rows == seg.cols == size
    return seg


# ---------------------------------------------------------------- 1. patterns

ODOM_Z = 0.2


@pytest.fixture(scope="module")
def pattern_scene():
    """one crafted cloud per pattern of cluster_ref.patterns, one point at the centre of every occupied cell, on fresh maps through a
    non-consecutive slot list; made once and shared: no call of this file changes a map"""
    import torch

    pats = cluster_ref.patterns(79, 79)
    names = list(pats)
    slots = [13, 2, 7, 0, 9, 4, 12, 1, 6, 10, 3, 15, 5, 11]
    assert len(slots) == len(names) == 14
    seg = small_chunk_context(16, 6400)
    seg.reset_maps(odom_z=ODOM_Z)
    length, res = GEOMETRY[79]
    ref = oracle.OracleMap(length, res, odom_z=ODOM_Z)
    rng = np.random.default_rng(5100)
    clouds, cells = [], []
    for name in names:
        rc = np.argwhere(pats[name])
        rc = rc[rng.permutation(len(rc))]  # (the points arrive in no particular order)
        x, y = cell_centres(ref, rc)
        clouds.append(cloud_of(x, y, rng.normal(0.5, 2.0, len(rc)).astype(np.float32)))
        cells.append(rc)
    n_pts = [len(c) for c in clouds]
    assert n_pts[names.index("empty")] == 0 and n_pts[names.index("full")] == 6241
    stride = stride_of(clouds)
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    labels = torch.full((len(names), stride), 99, dtype=torch.uint8, device="cuda")
    want = {}

    def expected(conn, order):
        if (conn, order) not in want:
            res_ = []
            for i in range(len(names)):
                h = clouds[i]["z"].astype(np.float32) - np.float32(ODOM_Z)
                res_.append(cluster_ref.expected_clusters(79, 79, cells[i][:, 0], cells[i][:, 1], h, np.ones(n_pts[i], bool), 1, conn, ORDER[order]))
            want[(conn, order)] = res_
        return want[(conn, order)]

    yield dict(seg=seg, names=names, slots=slots, pts=pts, labels=labels, n_pts=n_pts, stride=stride, expected=expected)
    seg.close()


@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("conn", [4, 8])
def test_patterns(pattern_scene, conn, order):
    import torch

    sc = pattern_scene
    seg, n, names = sc["seg"], len(sc["names"]), sc["names"]
    want = sc["expected"](conn, order)
    K = {name: want[i][1] for i, name in enumerate(names)}
    assert K["empty"] == 0 and K["full"] == 1 and K["checkerboard"] == (3121 if conn == 4 else 1) and K["spiral"] == 1
    assert K["comb"] == K["comb_t"] == K["u"] == K["w"] == 1 and K["corner_blocks"] == (4 if conn == 4 else 2) and K["trap"] == 4
    assert want[names.index("full")][2][0, 0] == 6241 and K["random_30"] > 256
    plane_stride = seg.rows * seg.cols + 3
    dst = Dest(n, plane_stride, sc["stride"], 256, slack=129)
    assert fresh_count(seg) == 16
    rc = raw_cluster(seg, n, sc["slots"], 0, _lib.GG_POINT16, sc["pts"].data_ptr(), sc["stride"], sc["n_pts"], dst, labels=sc["labels"].data_ptr(),
                     conn=conn, order=order)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 16
    host = dst.host()
    assert np.all(host["planes"][n * plane_stride:] == SENTINEL)
    for i, name in enumerate(names):
        check_cloud(host, i, want[i], sc["n_pts"][i], order, seg.rows, seg.cols, plane_stride, 256, f"{name} {conn} {ORDER[order]}")


# ---------------------------------------------------------------- 2. threshold and band

@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("band", [(-1.0, 2.0), (-INF, INF)])
def test_threshold_and_band(band, conn):
    import torch

    seg = small_chunk_context(1, 4096)
    seg.reset_maps(odom_z=0.0, on_torch_stream=True)  # (h = z - 0.0 = z, to the bit)
    length, res = GEOMETRY[79]
    ref = oracle.OracleMap(length, res, odom_z=0.0)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    tiny = list(np.array([1, 2, 0x007FFFFF, 0x80000001, 0x80000003], dtype=np.uint32).view(np.float32))  # denormals of both signs
    big = [0.0, -0.0, 1.25, -0.5, -1.0, 2.0, 2.5, -1.5, nan, inf, -inf, np.float32(-1.0000001), np.float32(2.0000002)] + tiny
    groups = [((10, 10), big * 2 + [0.5] * 4),           # 40 points: inside, on both bounds, below, above, NaN, both infinities, denormals
              ((10, 11), [0.1, 0.2, 0.3]),               # 3 points next to it
              ((20, 20), [0.4, 0.4]),                    # 2 points: below min_points
              ((20, 22), [1.0]),                         # 1 point
              ((30, 30), [nan] * 5),                     # NaN heights only: occupied, height_max is the quiet NaN
              ((40, 40), [0.5, 0.6, -7.0, -8.0]),        # 2 of 4 inside the band
              ((50, 50), [-1.0, 2.0, -1.0]),             # exactly on the bounds
              ((60, 60), [0.0, -0.0, -0.0]),             # only the two zeros
              ((61, 61), [-inf, -inf, -inf]),            # its diagonal neighbour
              ((70, 5), [-inf, nan, -inf, nan]),         # -inf and NaN only
              ((72, 40), [inf, 1.0, nan])]               # +inf
    rc = [cell for cell, zs in groups for _ in zs]
    x, y = cell_centres(ref, rc)
    z = np.array([v for _, zs in groups for v in zs], dtype=np.float32)
    assert len(groups[0][1]) == 40
    labels = np.full(len(z), 99, dtype=np.uint8)
    # points of other labels in a cell of their own (three of each: they would make it occupied) and in the big cell
    fx, fy = cell_centres(ref, [(65, 20)] * 9 + [(10, 10)] * 3)
    x, y, z = np.concatenate([x, fx]), np.concatenate([y, fy]), np.concatenate([z, np.full(12, 0.5, np.float32)])
    labels = np.concatenate([labels, np.array([49, 0, 7] * 4, dtype=np.uint8)])
    # selected points outside the map
    out_xy = [(1000.0, 0.0), (np.nan, 1.0), (2.0, np.inf), (-np.inf, np.nan), (0.0, -14.0)]
    assert not any(ref.get_index(float(a), float(b))[0] for a, b in out_xy)
    x = np.concatenate([x, np.array([a for a, _ in out_xy] * 3, np.float32)])
    y = np.concatenate([y, np.array([b for _, b in out_xy] * 3, np.float32)])
    z, labels = np.concatenate([z, np.full(15, 0.5, np.float32)]), np.concatenate([labels, np.full(15, 99, np.uint8)])
    n = len(z)
    perm = np.random.default_rng(5200).permutation(n)
    cloud = cloud_of(x[perm], y[perm], z[perm])
    labels = labels[perm]
    want = expectation(ref, cloud, labels, 3, band[0], band[1], conn, "row", ground=0.0)
    plane, K, table, ids = want
    finite = band[0] == -1.0
    assert plane[20, 20] == plane[20, 22] == plane[65, 20] == -1 and plane[10, 10] == plane[10, 11] == 0
    assert (plane[40, 40] == -1) == finite and (plane[61, 61] == -1) == finite and (plane[70, 5] == -1) == finite
    assert table[plane[30, 30], 6] == cluster_ref.QUIET_NAN and table[plane[30, 30], 1] == 5
    assert table[plane[60, 60], 6] == 0x00000000  # +0.0 above -0.0 (and above the -inf of its diagonal neighbour at 8)
    assert table[plane[50, 50], 6] == np.float32(2.0).view(np.uint32) and table[plane[50, 50], 1] == 3
    if not finite:
        assert table[plane[70, 5], 6] == np.float32(-np.inf).view(np.uint32) and table[0, 6] == np.float32(np.inf).view(np.uint32)
        assert (plane[61, 61] == plane[60, 60]) == (conn == 8)
    else:
        assert table[0, 6] == np.float32(2.0).view(np.uint32) and table[0, 1] == 40 - 2 * 6 + 3
    assert int(((ids == -1) & (labels == 99)).sum()) >= 18  # non-participating and unoccupied non-ground points
    stride = stride_of([cloud])
    pts = points_tensor([cloud], stride, _lib.GG_POINT16)
    d_labels = torch.from_numpy(np.concatenate([labels, np.full(stride - n, 99, np.uint8)])[None, :].copy()).cuda()
    plane_stride = seg.rows * seg.cols + 3
    dst = Dest(1, plane_stride, stride, 16)
    rc = raw_cluster(seg, 1, None, 0, _lib.GG_POINT16, pts.data_ptr(), stride, [n], dst, labels=d_labels.data_ptr(), min_points=3, lo=band[0], hi=band[1], conn=conn)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 1
    check_cloud(dst.host(), 0, want, n, ROW, seg.rows, seg.cols, plane_stride, 16, f"band {band} {conn}")
    seg.close()


# ---------------------------------------------------------------- 3. a real scan

SCAN = dict(min_points=2, lo=0.3, hi=2.5)


def cluster_scene(fmt, use_tf):
    """The scene of test_rasterize_clouds_gpu.raster_scene at 364 x 364: eleven maps through a non-consecutive slot list -- five warmed by two
    scrolled batches, six as the reset left them --, then one batch of distinct clouds of the lengths full (a 64-ring scan), 12000,
    4 * 128 + 1, 129, 128, 127, 65, 64, 63, 1, 0.  Returns the context, the batch's device tensors, the oracle maps and the map-frame clouds."""
    import torch

    length, res = GEOMETRY[364]
    slots = [11, 2, 7, 0, 9, 4, 12, 1, 6, 10, 3]
    seg = api.GroundSegmentation().init(length, res, n_slots=13, max_points=20000)
    seg.reset_maps(odom_z=0.2)
    refs = [oracle.OracleMap(length, res, odom_z=0.2) for _ in slots]
    warm_maps(seg, slots[:5], seed=5300, refs=refs[:5])
    assert fresh_count(seg) == 13 - 5
    extent = 0.6 * length
    clouds = [synth.hdl64_cloud(seed=5350, n_az=300), synth.random_cloud(12000, seed=5351, extent=extent)]
    clouds += [synth.random_cloud(m, seed=5360 + m, extent=extent) for m in (4 * 128 + 1, 129, 128, 127, 65, 64, 63, 1)]
    clouds.append(synth.empty_cloud(0))
    n_pts = [len(c) for c in clouds]
    assert n_pts[1:] == [12000, 513, 129, 128, 127, 65, 64, 63, 1, 0] and n_pts[0] > 12000
    stride = stride_of(clouds)
    R, t, tf = transform_of()
    maps = [kitti.transform_cloud(c, R, t) if len(c) else c for c in clouds] if use_tf else clouds
    origin = tuple(np.float32(v) for v in t) if use_tf else (0.0, 0.0, 0.0)
    pts = points_tensor(clouds, stride, fmt)
    out = seg.filter_batch(pts, n_pts, [origin] * len(slots), np.full(len(slots), -1.73), slots=slots, want_masks=True,
                           transforms=[tf] * len(slots) if use_tf else None)
    torch.cuda.synchronize()
    labels = out.labels.cpu().numpy()
    oracle_labels = []
    for i in range(len(slots)):
        r = refs[i].filter_cloud(maps[i], origin, -1.73)
        assert np.array_equal(labels[i, : n_pts[i]], r["label"]), f"cloud {i}: the batch's labels are not the oracle's"
        oracle_labels.append(r["label"])
    got_masks = out.label_masks.cpu().numpy()
    host_masks = masks_of(np.where(np.arange(stride)[None, :] < np.array(n_pts)[:, None], labels, 0).astype(np.uint8), stride)
    for i in range(len(slots)):
        assert np.array_equal(got_masks[i, : (n_pts[i] + 3) // 4], host_masks[i, : (n_pts[i] + 3) // 4]), f"cloud {i}: the batch's masks are not its labels"
    return dict(seg=seg, slots=slots, pts=pts, n_pts=n_pts, stride=stride, out=out, masks=out.label_masks, refs=refs, maps=maps, labels=oracle_labels,
                tf=[tf] * len(slots) if use_tf else None, fmt=fmt, want={})


@pytest.fixture(scope="module")
def scan_scenes():
    cache = {}

    def get(fmt, use_tf):
        if (fmt, use_tf) not in cache:
            cache[(fmt, use_tf)] = cluster_scene(fmt, use_tf)
        return cache[(fmt, use_tf)]

    yield get
    for sc in cache.values():
        sc["seg"].close()


@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("use_masks", [False, True])
@pytest.mark.parametrize("fmt", [_lib.GG_POINT16, _lib.GG_POINT32])
def test_a_real_scan(scan_scenes, fmt, use_masks, use_tf, order):
    import torch

    sc = scan_scenes(fmt, use_tf)
    seg, n = sc["seg"], len(sc["slots"])
    if order not in sc["want"]:
        sc["want"][order] = [expectation(sc["refs"][i], sc["maps"][i], sc["labels"][i], SCAN["min_points"], SCAN["lo"], SCAN["hi"], 8, ORDER[order]) for i in range(n)]
    want = sc["want"][order]
    # the scene holds what the test is about (on the oracle's expectation)
    sizes = np.concatenate([w[2][:, 0].view(np.int32) for w in want])
    assert int((sizes >= 2).sum()) >= 20, int((sizes >= 2).sum())
    assert int(sizes.max()) >= 30, int(sizes.max())
    lost = sum(int(((w[3] == -1) & (sc["labels"][i] == 99)).sum()) for i, w in enumerate(want))
    assert lost >= 200, lost
    fresh_before = fresh_count(seg)
    plane_stride = seg.rows * seg.cols + 3
    max_clusters = 1024
    dst = Dest(n, plane_stride, sc["stride"], max_clusters)
    lab = dict(masks=sc["masks"].data_ptr()) if use_masks else dict(labels=sc["out"].labels.data_ptr())
    rc = raw_cluster(seg, n, sc["slots"], 0, fmt, sc["pts"].data_ptr(), sc["stride"], sc["n_pts"], dst, transforms=sc["tf"], conn=8, order=order,
                     min_points=SCAN["min_points"], lo=SCAN["lo"], hi=SCAN["hi"], **lab)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    host = dst.host()
    tag = f"{'point16' if fmt else 'point32'} {'masks' if use_masks else 'labels'} {'tf' if use_tf else 'map frame'} {ORDER[order]}"
    for i in range(n):
        check_cloud(host, i, want[i], sc["n_pts"][i], order, seg.rows, seg.cols, plane_stride, max_clusters, tag)


# ---------------------------------------------------------------- 4. agreement with the path itself

def test_agreement_with_the_obstacle_count():
    import torch

    slots = [3, 0, 2]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    seg.reset_maps(odom_z=0.1)
    warm_maps(seg, slots, seed=5400)
    clouds = [synth.hdl64_cloud(seed=5450 + k, n_az=140 + 11 * k) for k in range(3)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    pts = batch_points(clouds, stride)
    out = seg.filter_batch(pts, n_pts, np.zeros((3, 3), np.float32), np.full(3, -1.73), slots=slots, want_masks=True)
    max_clusters = 8192
    row = seg.cluster_clouds(pts, n_pts, labels=out.labels, slots=slots, max_clusters=max_clusters)
    col = seg.cluster_clouds(pts, n_pts, masks=out.label_masks, slots=slots, max_clusters=max_clusters, order="col", connectivity=4)
    count_row = seg.rasterize_clouds(pts, n_pts, labels=out.labels, slots=slots, channels=["nonground_count"])
    count_col = seg.rasterize_clouds(pts, n_pts, labels=out.labels, slots=slots, channels=["nonground_count"], order="col")
    torch.cuda.synchronize()
    assert float(count_row.sum()) > 1000
    assert np.array_equal(row.cell_cluster.cpu().numpy() >= 0, count_row[:, 0].cpu().numpy() > 0)
    assert np.array_equal(col.cell_cluster.cpu().numpy() >= 0, count_col[:, 0].cpu().numpy() > 0)
    for res in (row, col):
        for b in range(3):
            K = int(res.n_clusters[b].item())
            assert 0 < K <= max_clusters
            table = res.table(b)
            assert len(table) == K and int(table["points"].sum()) == int(count_row[b].sum().item())
            assert int(table["cells"].sum()) == int((count_row[b] > 0).sum().item())
    seg.close()


# ---------------------------------------------------------------- 5. twice the same

def test_twice_the_same(pattern_scene):
    import torch

    sc = pattern_scene
    seg, names = sc["seg"], sc["names"]
    pick = [names.index("random_45"), names.index("full")]
    pts, labels = sc["pts"][pick].contiguous(), sc["labels"][pick].contiguous()
    n_pts, slots = [sc["n_pts"][i] for i in pick], [sc["slots"][i] for i in pick]
    plane_stride = seg.rows * seg.cols + 3
    for conn in (4, 8):
        dsts = [Dest(2, plane_stride, sc["stride"], 256) for _ in range(2)]
        for d in dsts:
            assert raw_cluster(seg, 2, slots, 0, _lib.GG_POINT16, pts.data_ptr(), sc["stride"], n_pts, d, labels=labels.data_ptr(), conn=conn) == 0
        torch.cuda.synchronize()
        a, b = dsts[0].host(), dsts[1].host()
        for key in a:
            assert np.array_equal(a[key], b[key]), f"{key} differs between two runs at connectivity {conn}"
        assert int(a["counts"][1]) == 1 and int(a["counts"][0]) > 1


# ---------------------------------------------------------------- 6. nothing changes

def test_nothing_changes():
    import torch

    slots = [4, 1, 5, 2]
    K = len(slots)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000) for _ in range(2)]
    base = [synth.hdl64_cloud(seed=5600 + k, n_az=150 + 7 * k) for k in range(K)]
    stride = stride_of(base)
    pts = [batch_points(base, stride), batch_points(base[::-1], stride)]
    n_pts = [[len(c) for c in base], [len(c) for c in base[::-1]]]
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    lazy = ["maxGroundHeight", "groundCandidates", "planeDist"]
    results = []
    for which, seg in enumerate(segs):
        seg.reset_maps(odom_z=0.1)
        seg.set_scoring(slots=slots)
        first = seg.filter_batch(pts[0], n_pts[0], origins, base_z, slots=slots, want_masks=True)
        assert lazy_count(seg) == K
        if which == 0:  # the clustering between the two batches, on every map of the context (two of them fresh)
            all_pts = torch.zeros((6, stride, 16), dtype=torch.uint8, device="cuda")
            all_labels = torch.full((6, stride), 99, dtype=torch.uint8, device="cuda")
            every = seg.cluster_clouds(all_pts, [stride] * 6, labels=all_labels, slots=list(range(6)), min_height=-100.0, max_height=100.0)
            seg.cluster_clouds(pts[0], n_pts[0], masks=first.label_masks, slots=slots, min_points=2, min_height=0.3, max_height=2.5)
        # the lazily kept layers are still pending behind the call: their first reader computes them, to the values of the twin
        assert lazy_count(seg) == K
        pending = seg.export_layers(lazy, slots=slots)
        assert lazy_count(seg) == 0
        second = seg.filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
        planes = seg.export_layers()
        torch.cuda.synchronize()
        if which == 0:  # (every point at the origin: one cell per map holds them all)
            assert np.array_equal(every.n_clusters.cpu().numpy(), np.ones(6, np.int32))
            assert np.array_equal(every.clusters[:, 0, :2].cpu().numpy(), np.tile(np.array([1, stride], np.int32), (6, 1)))
        results.append(dict(fresh=fresh_count(seg), pending=pending.cpu().numpy(), planes=planes.cpu().numpy(), labels=second.labels.cpu().numpy(),
                            index=second.out_index.cpu().numpy(), counts=second.counts.cpu().numpy(), scores=seg.scores_raw(),
                            positions=[seg.map(s).getPosition() for s in range(6)]))
    a, b = results
    assert a["fresh"] == b["fresh"] == 2
    assert same_bits(a["pending"], b["pending"]) and same_bits(a["planes"], b["planes"])
    assert a["planes"].shape[1] == len(LAYERS) == 11
    assert np.array_equal(a["counts"], b["counts"]) and a["positions"] == b["positions"]
    for k in range(K):
        assert np.array_equal(a["labels"][k, : n_pts[1][k]], b["labels"][k, : n_pts[1][k]]) and np.array_equal(a["index"][k, : n_pts[1][k]], b["index"][k, : n_pts[1][k]])
    assert np.array_equal(a["scores"][0], b["scores"][0]) and np.array_equal(a["scores"][1], b["scores"][1]) and a["scores"][0].sum() == 2 * K
    for seg in segs:
        seg.close()


# ---------------------------------------------------------------- 7. a caller's stream, past the ring, no host synchronisation

@pytest.mark.parametrize("halves", [False, True])
def test_on_a_caller_stream_past_the_ring(halves):
    import torch

    n_slots, slots = 4, [2, 1, 3, 0]  # both halves (boundary 2)
    K, rounds = len(slots), PARAM_RING + 2
    base = [synth.hdl64_cloud(seed=5700 + k, n_az=60 + 5 * k) for k in range(K)]
    stride = stride_of(base)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride)
    if halves:
        seg.set_flags(concurrent_halves=True)
        seg.debug_set_tuning("halves_min_clouds", 2)
    sets = [base, base[::-1]]
    pts = [batch_points(c, stride) for c in sets]
    n_pts = [[len(c) for c in cs] for cs in sets]
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    plane_stride = seg.rows * seg.cols + 3
    max_clusters = 2048
    dsts = [Dest(K, plane_stride, stride, max_clusters) for _ in range(rounds)]
    torch.cuda.synchronize()  # (the uploads and the fills ran on torch's default stream)
    stream = torch.cuda.Stream()
    batches = []
    with torch.cuda.stream(stream):
        seg.reset_maps(odom_z=0.0, on_torch_stream=True)
        for r in range(rounds):  # no synchronisation anywhere: every batch has its own label tensor, every call its own destinations
            batches.append(seg.filter_batch(pts[r % 2], n_pts[r % 2], origins, base_z, slots=slots))
            rc = raw_cluster(seg, K, slots, 0, _lib.GG_POINT16, pts[r % 2].data_ptr(), stride, n_pts[r % 2], dsts[r], labels=batches[r].labels.data_ptr(),
                             min_points=1, lo=0.2, hi=3.0)
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    for r in range(rounds):
        host = dsts[r].host()
        for i in range(K):
            cloud = sets[r % 2][i]
            lab = refs[i].filter_cloud(cloud, (0.0, 0.0, 0.0), -1.73)["label"]
            want = expectation(refs[i], cloud, lab, 1, 0.2, 3.0, 8, "row")
            assert 0 < want[1] <= max_clusters
            check_cloud(host, i, want, len(cloud), ROW, seg.rows, seg.cols, plane_stride, max_clusters, f"round {r}, halves {halves}")
    seg.close()


# ---------------------------------------------------------------- 8. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=4096)
    seg.reset_maps(odom_z=0.4)
    clouds = [synth.hdl64_cloud(seed=5800 + k, n_az=40) for k in range(2)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    assert stride <= 4096
    warm_maps(seg, [4, 1], seed=5810, frames=1, n_az=40)
    before = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    labels = torch.full((2, stride), 99, dtype=torch.uint8, device="cuda")
    cells = seg.rows * seg.cols
    dst = Dest(2, cells, stride, 64)
    P, Lb = pts.data_ptr(), labels.data_ptr()

    def call(n=2, slots=None, first=0, fmt=_lib.GG_POINT16, points=P, stride=stride, n_points=n_pts, labels=Lb, masks=0, **kw):
        return raw_cluster(seg, n, slots, first, fmt, points, stride, n_points, dst, labels=labels, masks=masks, **kw)

    x = _lib.GGCloudClusters()
    x.n = 2
    assert seg._L.gg_cluster_clouds(None, C.byref(x), None) == INVALID
    assert seg._L.gg_cluster_clouds(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    # the ten shared members, through the shared frame
    assert call(slots=[1, 1]) == INVALID
    assert call(points=0) == INVALID
    assert call(n_points=None) == INVALID
    assert call(fmt=2) == INVALID
    assert call(fmt=-1) == INVALID
    assert call(masks=Lb) == INVALID                 # both
    assert call(labels=0) == INVALID                 # neither
    assert call(labels=0, masks=Lb, stride=stride - 2, n_points=[10, 10]) == INVALID  # masks with a stride that is no multiple of 4
    assert call(n_points=[-1, 5]) == INVALID
    assert call(n_points=[5, stride + 1]) == INVALID
    assert call(n_points=[5, 4097]) == CAPACITY      # above max_points (and above the stride: the capacity is what is reported)
    assert call(stride=4096, n_points=[5, 4097]) == CAPACITY
    assert call(stride=4097) == CAPACITY
    assert call(slots=[1, 6]) == CAPACITY
    assert call(slots=[-1, 2]) == CAPACITY
    assert call(first=5) == CAPACITY
    assert call(first=-1) == CAPACITY
    # its own
    assert call(cell=0) == INVALID
    assert call(counts=0) == INVALID
    assert call(min_points=0) == INVALID
    assert call(min_points=-3) == INVALID
    assert call(conn=6) == INVALID
    assert call(conn=0) == INVALID
    assert call(order=2) == INVALID
    assert call(order=-1) == INVALID
    assert call(plane_stride=cells - 1) == INVALID
    assert call(max_clusters=-1) == INVALID
    assert call(max_clusters=0) == INVALID           # with d_clusters given
    assert call(lo=math.nan) == INVALID
    assert call(hi=math.nan) == INVALID
    assert call(n=0, points=0, n_points=None, labels=0, fmt=9, stride=10 ** 9, cell=0, counts=0, ids=0, table=0, min_points=-1, conn=5, order=7,
                plane_stride=0, max_clusters=-4, lo=math.nan) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel()
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    assert same_bits(before.cpu().numpy(), after.cpu().numpy())
    assert call(slots=[4, 1]) == 0, seg._L.gg_last_error(seg._ctx)  # ... and the same arguments without a mistake are accepted
    assert call(slots=[4, 1], table=0, max_clusters=0, ids=0) == 0, seg._L.gg_last_error(seg._ctx)  # (no table, no ids: both are optional)
    torch.cuda.synchronize()
    host = dst.host()
    assert fresh_count(seg) == fresh_before
    for i in range(2):
        K = int(host["counts"][i])
        assert 0 < K and np.all(host["table"][i, min(K, 64):] == SENTINEL)
        assert int(host["planes"][i * cells: (i + 1) * cells].view(np.int32).max()) == K - 1
        assert int(host["table"][i, : min(K, 64), 1].sum()) <= n_pts[i]
    seg.close()


# ---------------------------------------------------------------- 9. the Python entry point

def test_python_entry_point(pattern_scene):
    import torch

    sc = pattern_scene
    seg, n, slots, names = sc["seg"], len(sc["slots"]), sc["slots"], sc["names"]
    args = (sc["pts"], sc["n_pts"])
    a = seg.cluster_clouds(*args, labels=sc["labels"], slots=slots)
    assert isinstance(a, api.ClusterOutputs)
    for t, shape in ((a.cell_cluster, (n, seg.rows, seg.cols)), (a.n_clusters, (n,)), (a.clusters, (n, 256, 8)), (a.point_cluster, (n, sc["stride"]))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    masks = torch.from_numpy(masks_of(sc["labels"].cpu().numpy(), sc["stride"])).cuda()
    b = seg.cluster_clouds(*args, masks=masks, slots=slots, order="col", connectivity=4, max_clusters=0, point_clusters=False)
    assert tuple(b.cell_cluster.shape) == (n, seg.cols, seg.rows) and b.clusters is None and b.point_cluster is None
    again = seg.cluster_clouds(*args, masks=masks, slots=slots, order="col", connectivity=4, max_clusters=0, point_clusters=False, out=b)
    assert again is b
    own = seg.cluster_clouds(*args, labels=sc["labels"], slots=slots, connectivity=4, max_clusters=4000, on_torch_stream=False)
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, slots=slots)
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, labels=sc["labels"], masks=masks, slots=slots)
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, labels=sc["labels"], slots=slots, connectivity=6)
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, labels=sc["labels"], slots=slots, order="fortran")
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, labels=sc["labels"], slots=slots, out=api.ClusterOutputs(cell_cluster=torch.empty((n, seg.rows, seg.cols + 1), dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, labels=sc["labels"], slots=slots, out=api.ClusterOutputs(cell_cluster=torch.empty(a.cell_cluster.shape, dtype=torch.int64, device="cuda")))
    with pytest.raises(ValueError):
        seg.cluster_clouds(*args, labels=sc["labels"], slots=slots, max_clusters=0, out=a)  # (a table that is not asked for)
    torch.cuda.synchronize()
    seg.synchronize()
    want8, want4c, want4 = sc["expected"](8, ROW), sc["expected"](4, COL), sc["expected"](4, ROW)
    for i in range(n):
        assert np.array_equal(a.cell_cluster[i].cpu().numpy(), want8[i][0]), names[i]
        assert np.array_equal(b.cell_cluster[i].cpu().numpy().T, want4c[i][0]), names[i]
        assert int(a.n_clusters[i].item()) == want8[i][1] and int(b.n_clusters[i].item()) == want4c[i][1]
        assert np.array_equal(a.point_cluster[i, : sc["n_pts"][i]].cpu().numpy(), want8[i][3])
        t = own.table(i)
        assert t.dtype == api.CLUSTER_DTYPE and len(t) == min(want4[i][1], 4000) == want4[i][1]
        assert np.array_equal(t.view(np.uint32).reshape(-1, 8), want4[i][2])
        assert t["height_max"].dtype == np.float32
    k = names.index("random_30")
    assert len(a.table(k)) == 256 < want8[k][1]
