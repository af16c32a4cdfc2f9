"""gg_box_clusters (the oriented box of every obstacle cluster of many clouds: per cluster and candidate heading the extents of its points,
the heading of the smallest integer cost, a 32-byte record per cluster and the cost volume, in device memory, one call) on the device.
Expected values come from tests/box_ref.py (itself held by tests/test_box_clusters_cpu.py) fed with the downloaded ids and counts, the
maps' positions and the CPU oracle's own inside test (OracleMap.get_index).  Every comparison is on bits; there is no tolerance."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, kitti, synth  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import box_ref  # noqa: E402
from tests.box_ref import AREA, EDGE  # noqa: E402
from tests.test_export_layers_gpu import SENTINEL, fresh_count, same_bits, stride_of  # noqa: E402
from tests.test_split_clouds_gpu import GEOMETRY, lazy_count, points_tensor, transform_of  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, GEOMETRY_ERR, CAPACITY = -1, -2, -5
SIGNED_SENTINEL = SENTINEL - (1 << 32) if SENTINEL >= (1 << 31) else SENTINEL
SENTINEL64 = (SENTINEL << 32) | SENTINEL
SIDE = 79
LENGTH, RES = GEOMETRY[SIDE]
I32_MIN = -2 ** 31


def table_of(K):
    """K headings over [0, 90 degrees)"""
    return box_ref.rotation_table([k * (math.pi / 2) / K for k in range(K)])


# ---------------------------------------------------------------- helpers

class Dest:
    """sentinel-filled destinations of one call: the records and the cost volume"""

    def __init__(self, n, M, K):
        import torch

        self.n, self.M, self.K = n, M, K
        self.boxes = torch.full((n * M * 8,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.costs = torch.full((n * M * K * 2,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

    def host(self):
        return self.boxes.cpu().numpy().reshape(self.n, self.M, 8), self.costs.cpu().numpy().view(np.uint64).reshape(self.n, self.M, self.K)

    def all_sentinel(self):
        return bool((self.boxes == SIGNED_SENTINEL).all().item()) and bool((self.costs == SIGNED_SENTINEL).all().item())


def raw_box(seg, n, slots, first_slot, fmt, points, stride, n_points, ids, counts, rot, criterion, dest, transforms=None, costs=True, stream=None,
            own=False, **over):
    """gg_box_clusters as the C ABI has it (device addresses as integers, 0 = null); returns the status.  `over`: boxes, cost_ptr, K,
    max_clusters, rotations in place of what `dest` and `rot` give"""
    import torch

    x = _lib.GGClusterBoxes()
    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    npts = None if n_points is None else (C.c_int32 * max(len(n_points), 1))(*[int(v) for v in n_points])
    x.n, x.first_slot, x.slots, x.point_format = n, first_slot, sl, fmt
    x.d_points, x.cloud_stride, x.n_points = points or None, stride, npts
    tfs = None
    if transforms is not None:
        tfs = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(-1, 12))
        x.transforms = tfs.ctypes.data_as(C.POINTER(C.c_double))
    x.d_point_cluster, x.d_n_clusters = ids or None, counts or None
    table = np.ascontiguousarray(np.asarray(rot, dtype=np.int32).reshape(-1, 2))
    if over.get("rotations", True) is not None:
        x.rotations = table.ctypes.data_as(C.POINTER(C.c_int32))
    x.n_rotations = over.get("K", table.shape[0])
    x.criterion, x.max_clusters = criterion, over.get("max_clusters", dest.M)
    x.d_boxes = over.get("boxes", dest.boxes.data_ptr()) or None
    x.d_costs = over.get("cost_ptr", dest.costs.data_ptr() if costs else 0) or None
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_box_clusters(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def inside_of(ref, x, y, ids, Mi):
    """the oracle's inside test for the points whose id can select them (the others never participate)"""
    inside = np.zeros(len(ids), bool)
    for p in np.nonzero((ids >= 0) & (ids < Mi))[0]:
        ok, r, c = ref.get_index(float(x[p]), float(y[p]))
        inside[p] = ok and 0 <= r < ref.rows and 0 <= c < ref.cols
    return inside


def expect(position, cloud_map, ids, n_clusters, rot, criterion, M):
    """box_ref.expected_boxes of one cloud on a map at `position`: cloud_map the points in the map frame, ids its d_point_cluster words"""
    ref = oracle.OracleMap(LENGTH, RES, pos=position)
    assert ref.rows == ref.cols == SIDE and ref.position == tuple(position)
    n = len(cloud_map)
    Mi = min(max(int(n_clusters), 0), M)
    inside = inside_of(ref, cloud_map["x"], cloud_map["y"], ids[:n], Mi)
    return box_ref.expected_boxes(cloud_map["x"], cloud_map["y"], ids[:n], n_clusters, position, ref.resolution, rot, criterion, M, inside)


def check_cloud(boxes, costs, i, want, tag, with_costs=True):
    """cloud i of a downloaded Dest against an expectation: the records, the cost rows, and nothing written behind M_i"""
    Mi, rec, cost = want
    for k, name in enumerate(box_ref.FIELDS):
        bad = np.nonzero(boxes[i, :Mi, k] != rec[:, k])[0]
        assert len(bad) == 0, f"{tag}: cloud {i}: {name} of {len(bad)} records differs, first {bad[0]}: {boxes[i, bad[0]].tolist()} != {rec[bad[0]].tolist()}"
    assert np.all(boxes[i, Mi:] == SIGNED_SENTINEL), f"{tag}: cloud {i}: records behind M_i were written"
    if with_costs:
        bad = np.argwhere(costs[i, :Mi] != cost)
        assert len(bad) == 0, f"{tag}: cloud {i}: {len(bad)} costs differ, first {bad[0].tolist()}: {costs[i, bad[0][0], bad[0][1]]} != {cost[bad[0][0], bad[0][1]]}"
        assert np.all(costs[i, Mi:] == SENTINEL64), f"{tag}: cloud {i}: cost rows behind M_i were written"
    else:
        assert np.all(costs[i] == SENTINEL64), f"{tag}: cloud {i}: d_costs was not given and was written"


def cloud_at(position, ux, uy):
    """a cloud whose points lie at the centres of the units (ux, uy) of a map at `position`"""
    cloud = synth.empty_cloud(len(ux))
    cloud["x"] = (position[0] + (np.asarray(ux) + 0.5) * (np.float64(np.float32(RES)) / 16.0)).astype(np.float32)
    cloud["y"] = (position[1] + (np.asarray(uy) + 0.5) * (np.float64(np.float32(RES)) / 16.0)).astype(np.float32)
    cloud["z"] = 0.5
    return cloud


def device_i32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


# ---------------------------------------------------------------- 1. random scenes behind filter_batch and cluster_clouds

SLOTS = [5, 2, 7, 0, 3, 6]
POSITIONS = {5: (3.7, -1.9), 2: (3.7, -1.9), 7: (-12.25, 40.5), 0: (3.7, -1.9), 3: (0.013, 0.007), 6: (3.7, -1.9)}
MAXC = 256


@functools.lru_cache(maxsize=None)
def scene(fmt, use_tf):
    """Six clouds through a slot list onto maps at three positions: two sensor sweeps, a random cloud that exceeds the map, 129 points, no
    point, 1500 points; cloud_stride is larger than every n_points.  filter_batch labels them, cluster_clouds leaves the ids and the counts
    (and its own table) on the device.  Made once per (format, transforms); no test changes a map.  The contexts live as long as the
    module's cache."""
    import torch

    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=8, max_points=20000)
    assert seg.rows == seg.cols == SIDE
    seg.reset_maps(odom_z=0.2, pos=(3.7, -1.9))
    for s in (7, 3):
        seg.map(s).setPosition(*POSITIONS[s])
    positions = [tuple(seg.map(s).getPosition()) for s in SLOTS]
    assert positions == [POSITIONS[s] for s in SLOTS]
    R, t, tf = transform_of()
    clouds = []
    for i, s in enumerate(SLOTS):
        if i < 2:
            c = synth.hdl64_cloud(seed=6100 + i, n_az=130 + 20 * i)
        elif i == 4:
            c = synth.empty_cloud(0)
        else:
            c = synth.random_cloud((1500, 129, 0, 1500)[i - 2], seed=6110 + i, extent=0.6 * LENGTH)
            c["z"] = np.where(np.arange(len(c)) % 3 == 0, c["z"], np.float32(1.5)).astype(np.float32)  # (obstacles: most points stand above the ground)
        if len(c):  # around the map's position, in the frame the call is given the points in
            c["x"] += np.float32(positions[i][0])
            c["y"] += np.float32(positions[i][1])
            if use_tf:
                c = kitti.transform_cloud(c, R.T, -R.T @ t)  # (the sensor frame: the call's transform brings it back, up to rounding)
        clouds.append(c)
    n_pts = [len(c) for c in clouds]
    stride = stride_of(clouds) + 64
    maps = [kitti.transform_cloud(c, R, t) if len(c) else c for c in clouds] if use_tf else clouds  # what the path computes (Nodelet.cpp:166-181)
    pts = points_tensor(clouds, stride, fmt)
    tfs = [tf] * len(SLOTS) if use_tf else None
    origins = [tuple(np.float32(v) for v in (positions[i][0], positions[i][1], 0.0)) for i in range(len(SLOTS))]
    out = seg.filter_batch(pts, n_pts, origins, np.full(len(SLOTS), -1.73), slots=SLOTS, want_masks=True, transforms=tfs)
    cl = seg.cluster_clouds(pts, n_pts, labels=out.labels, transforms=tfs, slots=SLOTS, connectivity=4, max_clusters=MAXC)
    torch.cuda.synchronize()
    ids, counts = cl.point_cluster.cpu().numpy(), cl.n_clusters.cpu().numpy()
    print(f"scene {fmt} {use_tf}: n_points {n_pts}, clusters {counts.tolist()}")
    assert counts[4] == 0 and counts.sum() > 40 and (counts > 5).sum() >= 3, counts
    return dict(seg=seg, pts=pts, n_pts=n_pts, stride=stride, tfs=tfs, maps=maps, positions=positions, cl=cl, ids=ids, counts=counts, fmt=fmt)


@pytest.mark.parametrize("K", [1, 5, 32])
@pytest.mark.parametrize("criterion", [AREA, EDGE])
@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("fmt", [_lib.GG_POINT16, _lib.GG_POINT32])
def test_random_scenes(fmt, use_tf, criterion, K):
    import torch

    sc = scene(fmt, use_tf)
    seg, n = sc["seg"], len(SLOTS)
    rot = table_of(K) if K > 1 else box_ref.rotation_table([0.3])
    dst = Dest(n, MAXC, K)
    fresh, lazy = fresh_count(seg), lazy_count(seg)
    rc = raw_box(seg, n, SLOTS, 0, fmt, sc["pts"].data_ptr(), sc["stride"], sc["n_pts"], sc["cl"].point_cluster.data_ptr(), sc["cl"].n_clusters.data_ptr(),
                 rot, criterion, dst, transforms=sc["tfs"])
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert (fresh_count(seg), lazy_count(seg)) == (fresh, lazy)
    boxes, costs = dst.host()
    tag = f"{'point16' if fmt == _lib.GG_POINT16 else 'point32'} {'tf' if use_tf else 'map frame'} {'edge' if criterion else 'area'} K={K}"
    seen = 0
    for i in range(n):
        want = expect(sc["positions"][i], sc["maps"][i], sc["ids"][i], sc["counts"][i], rot, criterion, MAXC)
        check_cloud(boxes, costs, i, want, tag)
        seen += int((want[1][:, 1] > 1).sum())
    assert seen > 10, "the scene has too few clusters of several points"
    # the chained cross-check: with ids and counts as cluster_clouds left them, gg_box.points is gg_cluster.points
    table = sc["cl"].clusters.cpu().numpy()
    for i in range(n):
        m = min(int(sc["counts"][i]), MAXC)
        assert np.array_equal(boxes[i, :m, 1], table[i, :m, 1]), f"{tag}: cloud {i}: gg_box.points is not gg_cluster.points"
        assert np.all(boxes[i, :m, 0] >= 0)


def test_without_costs_and_twice_the_same_bytes():
    import torch

    sc = scene(_lib.GG_POINT16, False)
    seg, n, rot = sc["seg"], len(SLOTS), table_of(16)
    args = (seg, n, SLOTS, 0, sc["fmt"], sc["pts"].data_ptr(), sc["stride"], sc["n_pts"], sc["cl"].point_cluster.data_ptr(), sc["cl"].n_clusters.data_ptr(), rot)
    runs = []
    for crit in (EDGE, AREA):
        a, b, c = Dest(n, MAXC, 16), Dest(n, MAXC, 16), Dest(n, MAXC, 16)
        assert raw_box(*args, crit, a) == 0 and raw_box(*args, crit, b) == 0 and raw_box(*args, crit, c, costs=False, own=True) == 0
        seg.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(a.boxes, b.boxes) and torch.equal(a.costs, b.costs), "two runs of the same call differ"
        assert torch.equal(a.boxes, c.boxes) and bool((c.costs == SIGNED_SENTINEL).all().item()), "the records depend on d_costs, or a null d_costs was written"
        runs.append(a.host())
    assert not np.array_equal(runs[0][1], runs[1][1])  # (the two criteria are two volumes)


# ---------------------------------------------------------------- 2. crafted ids: slabs, hostile inputs, ties

@pytest.fixture(scope="module")
def plain():
    """a context of fresh maps at (0, 0) for the crafted clouds; no test changes a map"""
    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=4, max_points=8192)
    seg.reset_maps(odom_z=0.0)
    yield seg
    seg.close()


def run_crafted(seg, clouds, ids, counts, rot, criterion, M, fmt=_lib.GG_POINT16, tag="crafted", stride=None):
    """one call on crafted clouds (map frame, maps 0 .. n-1 at (0, 0)) with crafted ids and counts; held against the reference"""
    import torch

    n = len(clouds)
    stride = stride or stride_of(clouds)
    pts = points_tensor(clouds, stride, fmt)
    id_host = np.full((n, stride), SIGNED_SENTINEL, dtype=np.int32)
    for i, v in enumerate(ids):
        id_host[i, :len(v)] = v
    d_ids, d_counts = device_i32(id_host), device_i32(counts)
    dst = Dest(n, M, len(rot))
    assert fresh_count(seg) == 4
    rc = raw_box(seg, n, None, 0, fmt, pts.data_ptr(), stride, [len(c) for c in clouds], d_ids.data_ptr(), d_counts.data_ptr(), rot, criterion, dst)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 4
    boxes, costs = dst.host()
    wants = []
    for i in range(n):
        wants.append(expect((0.0, 0.0), clouds[i], id_host[i], counts[i], rot, criterion, M))
        check_cloud(boxes, costs, i, wants[-1], tag)
    return boxes, costs, wants


@pytest.mark.parametrize("criterion", [AREA, EDGE])
def test_slabs(plain, criterion):
    """a point per cell of a checkerboard: 3121 points; ids p % 700 with a count word of 3121 and max_clusters = 500: M_i = 500 clusters of
    four or five far-apart points each, three slabs of 191 at K = 32 (and one cloud of a single slab beside it)"""
    K, M = 32, 500
    S = _lib.box_slab_clusters(K, M)
    assert S == 191 and M > 2 * S
    rc = np.argwhere((np.add.outer(np.arange(SIDE), np.arange(SIDE)) % 2) == 0)
    rng = np.random.default_rng(6200)
    rc = rc[rng.permutation(len(rc))]
    assert len(rc) == 3121
    # cell (r, c) of an unmoved map spans the units [16 (half - r - 1), 16 (half - r)) with half = 39.5 cells
    ux = (16 * (SIDE / 2.0 - rc[:, 0] - 1) + rng.integers(0, 16, len(rc))).astype(np.int64)
    uy = (16 * (SIDE / 2.0 - rc[:, 1] - 1) + rng.integers(0, 16, len(rc))).astype(np.int64)
    cloud = cloud_at((0.0, 0.0), ux, uy)
    ids = (np.arange(len(rc)) % 700).astype(np.int32)
    small = cloud[:300].copy()
    boxes, costs, wants = run_crafted(plain, [cloud, small], [ids, ids[:300] % 150], [3121, 150], table_of(K), criterion, M, tag="slabs")
    assert wants[0][0] == 500 and np.all(wants[0][1][:, 1] >= 3) and wants[1][0] == 150 and np.all(wants[1][1][:, 1] == 2)
    assert len(np.unique(wants[0][1][:, 0])) > 8  # (many headings win somewhere)


def test_hostile_inputs(plain):
    rng = np.random.default_rng(6201)
    n = 400
    ux, uy = rng.integers(-500, 500, n), rng.integers(-500, 500, n)
    base = cloud_at((0.0, 0.0), ux, uy)
    ids = rng.integers(0, 12, n).astype(np.int32)
    ids[ids == 5] = 6                                        # a cluster id that no point carries
    ids[:6] = (-1, I32_MIN, 16, 17, 2 ** 31 - 1, -2)         # ids that select nothing
    hostile = base.copy()
    bad_xy = [(np.nan, 1.0), (2.0, np.inf), (-np.inf, np.nan), (1000.0, 0.0), (0.0, -13.1), (np.float32(3e38), np.float32(-3e38)), (np.nan, np.nan)]
    for j, (a, b) in enumerate(bad_xy):                      # coordinates that lie in no cell, under valid ids
        hostile["x"][10 + j], hostile["y"][10 + j] = a, b
    clouds = [base, base, hostile, base]
    counts = [-7, 10 ** 9, 16, 0]                            # negative: nothing; above max_clusters: all 16; the true count; none
    boxes, costs, wants = run_crafted(plain, clouds, [ids] * 4, counts, table_of(5), EDGE, 16, tag="hostile")
    assert [w[0] for w in wants] == [0, 16, 16, 0]
    assert np.all(boxes[0] == SIGNED_SENTINEL) and np.all(boxes[3] == SIGNED_SENTINEL) and np.all(costs[0] == SENTINEL64)
    for i in (1, 2):
        assert boxes[i, 5].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and np.all(costs[i, 5] == 2 ** 64 - 1)
        assert boxes[i, 12:].tolist() == [[-1, 0, 0, 0, 0, 0, 0, 0]] * 4     # ids 12 .. 15: below M_i, carried by no point
    assert boxes[1, :, 1].sum() == n - 6 and boxes[2, :, 1].sum() == n - 6 - len(bad_xy)


@pytest.mark.parametrize("fmt", [_lib.GG_POINT16, _lib.GG_POINT32])
def test_ties(plain, fmt):
    """a single-point cluster takes heading 0 with cost 0; the four corners of a square all lie on an edge at 0 and at 45 degrees: under
    EDGE 0 == 0 and the earlier table entry wins, whichever of the two it is"""
    cloud = cloud_at((0.0, 0.0), [100, 0, 8, 0, 8], [-200, 0, 0, 8, 8])
    ids = np.array([0, 1, 1, 1, 1], dtype=np.int32)
    d = box_ref.rotation_table([0.0, math.pi / 4])
    for rot, diag in ((d, False), (d[::-1].copy(), True)):
        boxes, costs, wants = run_crafted(plain, [cloud], [ids], [2], rot, EDGE, 4, fmt=fmt, tag="ties")
        assert boxes[0, 0, [0, 1, 6, 7]].tolist() == [0, 1, 0, 0] and boxes[0, 0, 2] == boxes[0, 0, 3] and boxes[0, 0, 4] == boxes[0, 0, 5]
        assert costs[0, :2].tolist() == [[0, 0], [0, 0]] and boxes[0, 1, :2].tolist() == [0, 4]
        assert boxes[0, 1, 2:6].tolist() == ([0, 16 * 11585, -8 * 11585, 8 * 11585] if diag else [0, 8 * 16384, 0, 8 * 16384])
    boxes, costs, wants = run_crafted(plain, [cloud], [ids], [2], d, AREA, 4, fmt=fmt, tag="ties area")
    assert boxes[0, 1, 0] == 0 and costs[0, 1].tolist() == [(8 * 16384) ** 2, (16 * 11585) ** 2] and boxes[0, 0, 0] == 0


# ---------------------------------------------------------------- 3. the maps

def test_no_map_changes():
    """the twin of a context that made the call between two batches computes the same layers, pending ones included"""
    import torch

    slots = [2, 0]
    clouds = [synth.hdl64_cloud(seed=6300 + k, n_az=90) for k in range(2)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    results = []
    for which in range(2):
        seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=4, max_points=stride)
        seg.reset_maps(odom_z=0.1)
        first = seg.filter_batch(pts, n_pts, np.zeros((2, 3), np.float32), np.full(2, -1.73), slots=slots)
        assert lazy_count(seg) == 2 and fresh_count(seg) == 2
        if which == 0:
            cl = seg.cluster_clouds(pts, n_pts, labels=first.labels, slots=slots)
            seg.box_clusters(pts, n_pts, cl.point_cluster, cl.n_clusters, table_of(16), slots=slots, costs=True, on_torch_stream=True)
            everything = torch.zeros((4, stride, 16), dtype=torch.uint8, device="cuda")
            zeros = torch.zeros((4, stride), dtype=torch.int32, device="cuda")
            seg.box_clusters(everything, [stride] * 4, zeros, torch.ones(4, dtype=torch.int32, device="cuda"), table_of(4), criterion="area", on_torch_stream=True)
            assert lazy_count(seg) == 2 and fresh_count(seg) == 2
        planes = seg.export_layers()
        torch.cuda.synchronize()
        results.append(dict(planes=planes.cpu().numpy(), positions=[seg.map(s).getPosition() for s in range(4)], fresh=fresh_count(seg)))
        seg.close()
    a, b = results
    assert same_bits(a["planes"], b["planes"]) and a["positions"] == b["positions"] and a["fresh"] == b["fresh"] == 2


# ---------------------------------------------------------------- 4. errors write nothing

def test_errors_write_nothing():
    import torch

    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=4, max_points=4096)
    seg.reset_maps(odom_z=0.0)
    rng = np.random.default_rng(6400)
    clouds = [cloud_at((0.0, 0.0), rng.integers(-400, 400, 200), rng.integers(-400, 400, 200)) for _ in range(2)]
    stride, n_pts = 256, [200, 200]
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    ids, counts = device_i32(rng.integers(0, 8, (2, stride))), device_i32([8, 8])
    rot = table_of(4)
    M = 8
    dst = Dest(2, M, 4)
    P, I, N = pts.data_ptr(), ids.data_ptr(), counts.data_ptr()

    def call(n=2, slots=None, first=0, fmt=_lib.GG_POINT16, points=P, stride=stride, n_points=n_pts, ids=I, counts=N, rot=rot, crit=EDGE, **over):
        return raw_box(seg, n, slots, first, fmt, points, stride, n_points, ids, counts, rot, crit, dst, **over)

    x = _lib.GGClusterBoxes()
    x.n = 2
    assert seg._L.gg_box_clusters(None, C.byref(x), None) == INVALID
    assert seg._L.gg_box_clusters(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(points=0) == INVALID and call(n_points=None) == INVALID and call(ids=0) == INVALID and call(counts=0) == INVALID
    assert call(boxes=0) == INVALID and call(rotations=None) == INVALID
    assert call(fmt=2) == INVALID and call(fmt=-1) == INVALID
    assert call(K=0) == INVALID and call(rot=table_of(33)) == INVALID and call(K=-1) == INVALID
    for word in (16385, -16385):
        bad = rot.copy()
        bad[2, 1] = word
        assert call(rot=bad) == INVALID
    assert call(max_clusters=0) == INVALID and call(max_clusters=4097) == INVALID and call(max_clusters=-1) == INVALID
    assert call(crit=2) == INVALID and call(crit=-1) == INVALID
    assert call(slots=[1, 1]) == INVALID                       # a repeated slot
    assert call(n_points=[-1, 5]) == INVALID and call(n_points=[5, stride + 1]) == INVALID
    assert call(n_points=[5, 4097]) == CAPACITY and call(stride=4097) == CAPACITY
    assert call(slots=[1, 4]) == CAPACITY and call(first=3) == CAPACITY and call(first=-1) == CAPACITY
    # overlapping buffers: an output on an input, an output on the other output
    assert call(boxes=I) == INVALID and call(boxes=P) == INVALID and call(boxes=N) == INVALID
    assert call(cost_ptr=I) == INVALID and call(cost_ptr=dst.boxes.data_ptr()) == INVALID
    assert call(boxes=dst.costs.data_ptr() + 8) == INVALID
    assert call(boxes=I + 4 * (2 * stride - 1)) == INVALID      # the last word of the ids
    assert call(n=0, points=0, n_points=None, ids=0, counts=0, K=99, crit=7, max_clusters=-3, boxes=0) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel() and fresh_count(seg) == 4
    assert call() == 0, seg._L.gg_last_error(seg._ctx)          # ... and the same arguments without a mistake are accepted
    torch.cuda.synchronize()
    boxes, costs = dst.host()
    host_ids = ids.cpu().numpy()
    for i in range(2):
        check_cloud(boxes, costs, i, expect((0.0, 0.0), clouds[i], host_ids[i], 8, rot, EDGE, M), "after the errors")
    seg.close()


def test_a_map_of_more_than_4096_cells_a_side_is_refused():
    """A context with a side of 4097 cells is refused with GG_ERR_GEOMETRY -- by gg_create already, whose own limits (the sweep's tables in
    local memory) end far below the 4096 cells the call's arithmetic allows: the call's own refusal (BOX_MAX_SIDE of gg_internal.h, held
    to that arithmetic by a static_assert there) cannot be reached through a context today.  No kernel is launched for such a map: there is no context to launch on."""
    geom = _lib.GGGeometry(4097.0, 1.0, 0.0, 0.0)
    ctx = C.c_void_p()
    L = _lib.load()
    assert L.gg_create(C.byref(geom), 1, 64, 0, C.byref(ctx)) == GEOMETRY_ERR and not ctx.value
    with pytest.raises(api.GroundGridError, match="GG_ERR_GEOMETRY"):
        api.GroundSegmentation().init(4097.0, 1.0, n_slots=1, max_points=64)
    x = _lib.GGClusterBoxes()
    x.n = 1
    assert L.gg_box_clusters(ctx, C.byref(x), None) == INVALID  # (the null context that gg_create left)


# ---------------------------------------------------------------- 5. the Python entry point

def test_python_entry_point():
    import torch

    sc = scene(_lib.GG_POINT16, True)
    seg, n, stride, cl = sc["seg"], len(SLOTS), sc["stride"], sc["cl"]
    rot = api.rotation_table([k * (math.pi / 2) / 16 for k in range(16)])
    a = seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, transforms=sc["tfs"], slots=SLOTS, max_clusters=MAXC, costs=True)
    assert a.boxes.shape == (n, MAXC, 8) and a.boxes.dtype == torch.int32 and a.boxes.is_cuda
    assert a.costs.shape == (n, MAXC, 16) and a.costs.dtype == torch.int64
    b = seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, transforms=sc["tfs"], slots=SLOTS, criterion="area", max_clusters=MAXC,
                         on_torch_stream=True)
    assert b.costs is None
    seg.synchronize()  # (a ran on the context's own stream; the fill runs on torch's)
    a.boxes.fill_(SIGNED_SENTINEL)
    again = seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, transforms=sc["tfs"], slots=SLOTS, max_clusters=MAXC, costs=True,
                             out=a, on_torch_stream=True)
    assert again is a
    seg.synchronize()
    torch.cuda.synchronize()
    for res, crit in ((a, EDGE), (b, AREA)):
        boxes = res.boxes.cpu().numpy()
        for i in range(n):
            Mi, rec, cost = expect(sc["positions"][i], sc["maps"][i], sc["ids"][i], sc["counts"][i], rot, crit, MAXC)
            assert np.array_equal(boxes[i, :Mi], rec), (crit, i)
            if res.costs is not None:
                assert np.array_equal(res.costs[i, :Mi].cpu().numpy().view(np.uint64), cost), (crit, i)
    m = a.metric(0, rot, RES, sc["positions"][0])
    k = min(int(sc["counts"][0]), MAXC)
    assert m.shape == (MAXC, 5) and np.isfinite(m[:k]).all() and np.all(m[:k, 2:4] >= 0)
    assert np.all(np.abs(m[:k, 0] - sc["positions"][0][0]) <= 0.5 * LENGTH + RES) and np.all(np.abs(m[:k, 1] - sc["positions"][0][1]) <= 0.5 * LENGTH + RES)
    common = dict(transforms=sc["tfs"], slots=SLOTS)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, criterion="hull", **common)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, max_clusters=4097, **common)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, np.zeros((33, 2), np.int32), **common)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, [[16385, 0]], **common)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster.to(torch.int64), cl.n_clusters, rot, **common)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters[:3], rot, **common)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, max_clusters=MAXC, out=a, **common)  # (a.costs is not asked for)
    with pytest.raises(ValueError):
        seg.box_clusters(sc["pts"], sc["n_pts"], cl.point_cluster, cl.n_clusters, rot, max_clusters=MAXC, out=api.BoxOutputs(boxes=cl.point_cluster), **common)
