"""gg_visibility_clouds (free, unknown and occupied cells of many labelled clouds by ray tracing, in device memory, one call) on the device.
Expected values come from numpy alone (tests/visibility_ref.py: the closed form of the header, itself held against exact rational arithmetic
by tests/test_visibility_clouds_cpu.py) on an occupancy and a set of hit cells that are a crafted scene or the CPU oracle's
(visibility_ref.cloud_truth: tests/test_cluster_clouds_gpu.expectation and OracleMap.get_index).  Every comparison is on bits; there is no
tolerance and no cell is left out."""
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
from tests import clearance_ref, visibility_ref  # noqa: E402
from tests.test_clearance_clouds_gpu import BAND, pattern_cloud, plain_context  # noqa: E402
from tests.test_cluster_clouds_gpu import cell_centres, cloud_of, small_chunk_context  # noqa: E402
from tests.test_export_layers_gpu import SENTINEL, batch_points, fresh_count, same_bits, stride_of, warm_maps  # noqa: E402
from tests.test_split_clouds_gpu import GEOMETRY, PARAM_RING, lazy_count, masks_of, points_tensor, transform_of  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
SIGNED_SENTINEL = SENTINEL - (1 << 32) if SENTINEL >= (1 << 31) else SENTINEL
INF = math.inf
FREE, UNKNOWN, OCCUPIED = visibility_ref.FREE, visibility_ref.UNKNOWN, visibility_ref.OCCUPIED
ODOM_Z = 0.2


# ---------------------------------------------------------------- helpers

class Dest:
    """sentinel-filled destinations of one call: n state planes plane_stride words apart (and `slack` words behind), and the counts"""

    def __init__(self, n, plane_stride, slack=0):
        import torch

        self.n, self.plane_stride = n, plane_stride
        self.state = torch.full((max(n * plane_stride + slack, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.counts = torch.full((max(3 * n, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

    def host(self):
        return dict(state=self.state.cpu().numpy().view(np.uint32), counts=self.counts.cpu().numpy().view(np.uint32).reshape(-1, 3))

    def all_sentinel(self):
        return bool((self.state == SIGNED_SENTINEL).all().item()) and bool((self.counts == SIGNED_SENTINEL).all().item())


def raw_visibility(seg, n, dest, origins, slots=None, first_slot=0, fmt=_lib.GG_POINT16, points=0, stride=0, n_points=None, labels=0, masks=0,
                   transforms=None, min_points=1, lo=-INF, hi=INF, max_cells=0, order=ROW, stream=None, own=False, **over):
    """gg_visibility_clouds as the C ABI has it (device addresses as integers, 0 = null; origins: [n][3] or None); returns the status.
    `over`: state, plane_stride, counts in place of what `dest` gives"""
    import torch

    x = _lib.GGCloudVisibility()
    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    npts = None if n_points is None else (C.c_int32 * max(len(n_points), 1))(*[int(v) for v in n_points])
    x.n, x.first_slot, x.slots, x.point_format = n, first_slot, sl, fmt
    x.d_points, x.cloud_stride, x.n_points = points or None, stride, npts
    tfs = None
    if transforms is not None:
        tfs = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(-1, 12))
        x.transforms = tfs.ctypes.data_as(C.POINTER(C.c_double))
    x.d_labels, x.d_label_masks = labels or None, masks or None
    x.min_points, x.min_height, x.max_height = min_points, lo, hi
    org = None
    if origins is not None:
        org = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
        x.origins = org.ctypes.data_as(C.POINTER(C.c_float))
    x.max_cells, x.order = max_cells, order
    x.d_state = over.get("state", dest.state.data_ptr()) or None
    x.plane_stride = over.get("plane_stride", dest.plane_stride)
    x.d_counts = over.get("counts", dest.counts.data_ptr()) or None
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_visibility_clouds(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check_cloud(host, i, want, rows, cols, plane_stride, tag, counts=True):
    """cloud i of a downloaded Dest against an expectation (state laid out as the library lays it out, counts): every cell, the three counts,
    the words behind the plane, and the counts of a call that handed none over"""
    state, want_counts = want
    at = i * plane_stride
    got = host["state"][at: at + rows * cols].view(np.int32).reshape(state.shape)
    bad = np.argwhere(got != state)
    assert len(bad) == 0, f"{tag}: cloud {i}: {len(bad)} cells differ, first {tuple(bad[0])}: {got[tuple(bad[0])]} != {state[tuple(bad[0])]}"
    assert np.all(host["state"][at + rows * cols: at + plane_stride] == SENTINEL), f"{tag}: cloud {i}: the words behind the plane were written"
    if counts:
        assert host["counts"][i].view(np.int32).tolist() == want_counts.tolist(), f"{tag}: cloud {i}: counts {host['counts'][i].view(np.int32)} != {want_counts}"
        assert int(want_counts.sum()) == rows * cols
    else:
        assert np.all(host["counts"][i] == SENTINEL), f"{tag}: cloud {i}: the counts were not handed over and were written"


def sensor_xy(ref, sensor):
    """the map-frame (x, y, z) of a scene's sensor: the centre of its cell, a point beyond the map, a NaN"""
    if sensor == visibility_ref.OUTSIDE:
        assert not ref.get_index(1000.0, 0.0)[0]
        return (1000.0, 0.0, 1.5)
    if sensor == visibility_ref.NOT_FINITE:
        return (np.nan, 0.0, 1.5)
    x, y = cell_centres(ref, [sensor])
    return (float(x[0]), float(y[0]), 1.5)


OUT_XY = [(1000.0, 0.0), (np.nan, 1.0), (2.0, np.inf), (-np.inf, np.nan), (0.0, -14.0)]  # in no 79 x 79 map


def scene_cloud(ref, name, scene, rng):
    """(map-frame cloud, label bytes) of a scene of visibility_ref.scenes: two non-ground points per occupied cell, one ground point per
    ground cell, one non-ground point per single cell; and what contributes nothing: points of other label bytes in the sensor's own row and
    in hit cells, and ground and non-ground points outside the map.  In no particular order."""
    if name == "empty":
        return synth.empty_cloud(0), np.zeros(0, np.uint8)
    cells = [c for c in scene["occupied"] for _ in range(2)] + scene["ground"] + scene["single"]
    lab = [99] * (2 * len(scene["occupied"])) + [49] * len(scene["ground"]) + [99] * len(scene["single"])
    other = [(1, 40), (40, 1), (77, 77)] + cells[:3]  # other label bytes: 0, 7, 98, 50, 255, 1
    cells, lab = cells + other, lab + [0, 7, 98, 50, 255, 1][: len(other)]
    if name == "all_outside":
        cells, lab = [], []
    x, y = cell_centres(ref, cells) if cells else (np.zeros(0, np.float32), np.zeros(0, np.float32))
    x = np.concatenate([x, np.array([a for a, _ in OUT_XY] * 2, np.float32)])
    y = np.concatenate([y, np.array([b for _, b in OUT_XY] * 2, np.float32)])
    lab = np.array(lab + [99] * len(OUT_XY) + [49] * len(OUT_XY), np.uint8)
    perm = rng.permutation(len(lab))
    return cloud_of(x[perm], y[perm], np.full(len(lab), 0.5, np.float32)), lab[perm]


# ---------------------------------------------------------------- 1. patterns

@pytest.fixture(scope="module")
def pattern_scene():
    """one crafted cloud per scene of visibility_ref.scenes on fresh 79 x 79 maps of a GG_PW=128 context, through a non-consecutive slot
    list; made once and shared: no call of this file changes a map"""
    import torch

    S = visibility_ref.scenes(79)
    names = list(S)
    n = len(names)
    assert n == 20
    slots = [int(s) for s in np.random.default_rng(7200).permutation(24)[:n]]
    length, res = GEOMETRY[79]
    ref = oracle.OracleMap(length, res, odom_z=ODOM_Z)
    assert not any(ref.get_index(float(a), float(b))[0] for a, b in OUT_XY)
    rng = np.random.default_rng(7210)
    made = [scene_cloud(ref, name, S[name], rng) for name in names]
    clouds, labels = [m[0] for m in made], [m[1] for m in made]
    n_pts = [len(c) for c in clouds]
    assert n_pts[names.index("empty")] == 0 and n_pts[names.index("all_outside")] == 2 * len(OUT_XY) and max(n_pts) > 4 * 128
    stride = stride_of(clouds)
    seg = small_chunk_context(24, stride)
    seg.reset_maps(odom_z=ODOM_Z)
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    host_labels = np.zeros((n, stride), np.uint8)
    for i, lab in enumerate(labels):
        host_labels[i, : len(lab)] = lab
    origins = np.array([sensor_xy(ref, S[name]["sensor"]) for name in names], np.float32)
    truth = [visibility_ref.scene_truth(S[name], 79) for name in names]
    want = {}

    def expected(max_cells, order):
        if (max_cells, order) not in want:
            want[(max_cells, order)] = [visibility_ref.expected_visibility(*truth[i], max_cells, ORDER[order]) for i in range(n)]
        return want[(max_cells, order)]

    yield dict(seg=seg, names=names, slots=slots, pts=pts, labels=torch.from_numpy(host_labels).cuda(), host_labels=host_labels, n_pts=n_pts, stride=stride,
               origins=origins, truth=truth, expected=expected, scenes=S)
    seg.close()


def pattern_call(sc, dst, pick=None, **kw):
    """the pattern scene's clouds `pick` (all of them) through raw_visibility under min_points = 2; returns (status, what must stay alive)"""
    if pick is None:
        pts, lab, n_pts, slots, origins = sc["pts"], sc["labels"], sc["n_pts"], sc["slots"], sc["origins"]
    else:
        pts, lab = sc["pts"][pick].contiguous(), sc["labels"][pick].contiguous()
        n_pts, slots, origins = [sc["n_pts"][i] for i in pick], [sc["slots"][i] for i in pick], sc["origins"][pick]
    rc = raw_visibility(sc["seg"], len(n_pts), dst, origins, slots=slots, points=pts.data_ptr(), stride=sc["stride"], n_points=n_pts, labels=lab.data_ptr(),
                        min_points=2, **kw)
    return rc, (pts, lab)


@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("max_cells", [0, 1, 7, 200])
def test_patterns(pattern_scene, max_cells, order):
    import torch

    sc = pattern_scene
    seg, names, n = sc["seg"], sc["names"], len(sc["names"])
    want = sc["expected"](max_cells, order)
    # the scenes hold what the test is about (on the expectation)
    row = {name: visibility_ref.expected_visibility(*sc["truth"][i], max_cells, "row")[0] for i, name in enumerate(names)}
    m = 39
    through = row["through_occupied"]
    assert through[m, m + 11] == OCCUPIED and through[m, m + 21] == FREE and through[m, m] == FREE
    assert through[m, m + 15] == (FREE if max_cells in (0, 200) else UNKNOWN)  # behind the occupied cell, on the way to the ground return
    assert row["single_nonground"][10, 50] == FREE and not (row["single_nonground"] == OCCUPIED).any()
    assert (row["end_is_sensor"] != UNKNOWN).sum() == 1 and row["end_is_sensor"][20, 20] == FREE
    for name in ("sensor_outside", "sensor_not_finite"):
        occupied, hit, origin = sc["truth"][names.index(name)]
        assert origin is None and np.array_equal(row[name] == FREE, hit & ~occupied)
    assert (row["empty"] == UNKNOWN).all() and (row["all_outside"] == UNKNOWN).all()
    if max_cells == 0:
        assert row["corner_00"][39, 39] == FREE and row["corner_rc"][39, 39] == FREE and row["halves_rows"][m + 1, m + 1] == FREE
        ring = row["ring"]  # nothing beyond the ring is free, and inside it nearly every cell is
        rr, cc = np.mgrid[0:79, 0:79]
        dist = np.hypot(rr - m, cc - m)
        assert not (ring[dist > 21] != UNKNOWN).any() and (ring[dist < 19] == FREE).mean() > 0.9 and not (ring[dist < 19] == OCCUPIED).any()
    plane_stride = seg.rows * seg.cols + 3
    dst = Dest(n, plane_stride, slack=129)
    assert fresh_count(seg) == 24
    rc, keep = pattern_call(sc, dst, max_cells=max_cells, order=order)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 24
    host = dst.host()
    assert np.all(host["state"][n * plane_stride:] == SENTINEL)
    for i, name in enumerate(names):
        check_cloud(host, i, want[i], 79, 79, plane_stride, f"{name} R={max_cells} {ORDER[order]}")


def test_without_counts(pattern_scene):
    import torch

    sc = pattern_scene
    seg, names = sc["seg"], sc["names"]
    pick = [names.index(k) for k in ("random", "empty", "ring")]
    want = sc["expected"](0, ROW)
    cells = 79 * 79
    dst = Dest(3, cells)
    rc, keep = pattern_call(sc, dst, pick, counts=0)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    for j, i in enumerate(pick):
        check_cloud(host, j, want[i], 79, 79, cells, f"no counts, {names[i]}", counts=False)


def test_many_clouds_one_share_each(pattern_scene):
    """260 clouds in one call: from 257 clouds on a cloud is traced by a single work-group (the shape of a batch of 1024)"""
    import torch

    sc = pattern_scene
    names, n = sc["names"], len(sc["names"])
    times = 13
    N = n * times
    seg = small_chunk_context(N, sc["stride"])
    seg.reset_maps(odom_z=ODOM_Z)
    slots = [int(s) for s in np.random.default_rng(7250).permutation(N)]
    pts, lab = sc["pts"].repeat(times, 1, 1).contiguous(), sc["labels"].repeat(times, 1).contiguous()
    cells = 79 * 79
    dst = Dest(N, cells + 1)
    rc = raw_visibility(seg, N, dst, np.tile(sc["origins"], (times, 1)), slots=slots, points=pts.data_ptr(), stride=sc["stride"], n_points=sc["n_pts"] * times,
                        labels=lab.data_ptr(), min_points=2, order=COL)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host, want = dst.host(), sc["expected"](0, COL)
    for i in range(N):
        check_cloud(host, i, want[i % n], 79, 79, cells + 1, f"cloud {i} of {N}, {names[i % n]}")
    seg.close()


# ---------------------------------------------------------------- 2. cloud variants

VARIANT_PATTERNS = ["random_30", "pairs", "spiral", "borders", "four_corners", "empty"]


@pytest.fixture(scope="module")
def variant_scene():
    """crafted clouds with a height band (tests/test_clearance_clouds_gpu.pattern_cloud: two points inside the band in occupied cells, and in
    other cells points below and above the band, single points and other labels), on fresh maps; one cloud is handed over empty and one
    has every point outside its map.  Every cloud has a sensor of its own.  Per use_tf the clouds as the caller gives them and the oracle's
    truth, made once"""
    pats = clearance_ref.patterns(79, 79)
    length, res = GEOMETRY[79]
    ref = oracle.OracleMap(length, res, odom_z=ODOM_Z)
    rng = np.random.default_rng(7300)
    made = [pattern_cloud(ref, pats[name], rng) for name in VARIANT_PATTERNS]
    map_clouds, labels = [m[0] for m in made], [m[1] for m in made]
    k = VARIANT_PATTERNS.index("empty")  # its points: outside the map, ground and non-ground
    map_clouds[k] = cloud_of(np.array([a for a, _ in OUT_XY] * 2, np.float32), np.array([b for _, b in OUT_XY] * 2, np.float32), np.full(2 * len(OUT_XY), 0.9, np.float32))
    labels[k] = np.array([99] * len(OUT_XY) + [49] * len(OUT_XY), np.uint8)
    n_pts = [len(c) for c in map_clouds]
    n_pts[VARIANT_PATTERNS.index("four_corners")] = 0  # handed over with n_points = 0
    stride = stride_of(map_clouds)
    seg = small_chunk_context(10, stride)
    seg.reset_maps(odom_z=ODOM_Z)
    R, t, tf = transform_of()
    sensors = [(39, 39), (0, 0), (78, 40), (20, 60), (5, 5), (39, 39)]
    origins = np.array([sensor_xy(ref, s) for s in sensors], np.float32)
    cache = {}

    def variant(use_tf):
        if use_tf not in cache:
            given = map_clouds
            if use_tf:  # the sensor-frame clouds whose transform lands in the same cells (half a cell of margin against the rounding)
                given = []
                for c in map_clouds:
                    s = c.copy()
                    if len(c):
                        with np.errstate(invalid="ignore"):  # (the points that are not finite stay so)
                            p = (np.stack([c["x"], c["y"], c["z"]], axis=1).astype(np.float64) - t) @ R
                        s["x"], s["y"], s["z"] = p[:, 0].astype(np.float32), p[:, 1].astype(np.float32), p[:, 2].astype(np.float32)
                    given.append(s)
            with np.errstate(invalid="ignore"):
                in_map = [kitti.transform_cloud(c, R, t) if use_tf and len(c) else c for c in given]
            truth = [visibility_ref.cloud_truth(ref, in_map[i][: n_pts[i]], labels[i], origins[i], 2, BAND[0], BAND[1], ground=ODOM_Z) for i in range(len(given))]
            for i, tr in enumerate(truth):
                assert tr[2] == sensors[i]
            cache[use_tf] = dict(given=given, truth=truth, tf=[tf] * len(given) if use_tf else None, want={})
        return cache[use_tf]

    host_labels = np.zeros((len(made), stride), np.uint8)
    for i, lab in enumerate(labels):
        host_labels[i, : len(lab)] = lab
    yield dict(seg=seg, variant=variant, n_pts=n_pts, stride=stride, labels=host_labels, origins=origins)
    seg.close()


@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("use_masks", [False, True])
@pytest.mark.parametrize("fmt", [_lib.GG_POINT16, _lib.GG_POINT32])
def test_cloud_variants(variant_scene, fmt, use_masks, use_tf):
    import torch

    sc, v = variant_scene, variant_scene["variant"](use_tf)
    seg, n, stride, n_pts = sc["seg"], len(VARIANT_PATTERNS), sc["stride"], sc["n_pts"]
    order = COL if use_masks else ROW
    max_cells = 25 if fmt == _lib.GG_POINT32 else 0
    if (max_cells, order) not in v["want"]:
        v["want"][(max_cells, order)] = [visibility_ref.expected_visibility(*tr, max_cells, ORDER[order]) for tr in v["truth"]]
    want = v["want"][(max_cells, order)]
    occupied, hits = [tr[0] for tr in v["truth"]], [tr[1] for tr in v["truth"]]
    assert int(occupied[0].sum()) > 1000 and int((hits[0] & ~occupied[0]).sum()) > 100  # hits the band or the threshold keeps from being occupied
    assert not hits[VARIANT_PATTERNS.index("empty")].any() and not hits[VARIANT_PATTERNS.index("four_corners")].any()
    pts = points_tensor(v["given"], stride, fmt)
    lab = torch.from_numpy(masks_of(sc["labels"], stride) if use_masks else sc["labels"]).cuda()
    which = dict(masks=lab.data_ptr()) if use_masks else dict(labels=lab.data_ptr())
    where = dict(slots=None, first_slot=3) if use_masks else dict(slots=[8, 2, 7, 0, 6, 3])
    plane_stride = seg.rows * seg.cols + 3
    dst = Dest(n, plane_stride)
    assert fresh_count(seg) == 10
    rc = raw_visibility(seg, n, dst, sc["origins"], fmt=fmt, points=pts.data_ptr(), stride=stride, n_points=n_pts, transforms=v["tf"], min_points=2, lo=BAND[0],
                        hi=BAND[1], max_cells=max_cells, order=order, **which, **where)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 10
    host = dst.host()
    tag = f"{'point16' if fmt else 'point32'} {'masks' if use_masks else 'labels'} {'tf' if use_tf else 'map frame'} {ORDER[order]}"
    for i, name in enumerate(VARIANT_PATTERNS):
        check_cloud(host, i, want[i], 79, 79, plane_stride, f"{tag} {name}")


# ---------------------------------------------------------------- 3. sizes

def test_a_side_that_is_no_multiple_of_64():
    import torch

    size = 148
    seg = plain_context(size, 2, max_points=2048)
    seg.reset_maps(odom_z=ODOM_Z)
    ref = oracle.OracleMap(49.0, 0.33, odom_z=ODOM_Z)
    assert ref.rows == ref.cols == size
    rng = np.random.default_rng(7400)
    sensors = [(5, 140), (147, 0)]
    clouds, labels, truth = [], [], []
    for k in range(2):
        cells = np.stack(np.unravel_index(rng.choice(size * size, 300, replace=False), (size, size)), axis=1)
        cells = np.concatenate([cells, [[147, 147], [0, 0], [0, 147], [147, 0], [77, 64]]])
        lab = rng.choice(np.array([49, 99], np.uint8), len(cells))
        x, y = cell_centres(ref, cells)
        clouds.append(cloud_of(x, y, np.full(len(cells), 0.7, np.float32)))
        labels.append(lab)
        occupied, hit = np.zeros((size, size), bool), np.zeros((size, size), bool)
        hit[cells[:, 0], cells[:, 1]] = True
        occupied[cells[lab == 99, 0], cells[lab == 99, 1]] = True
        truth.append((occupied, hit, sensors[k]))
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    host_labels = np.zeros((2, stride), np.uint8)
    for i, lab in enumerate(labels):
        host_labels[i, : len(lab)] = lab
    d_labels = torch.from_numpy(host_labels).cuda()
    origins = np.array([sensor_xy(ref, s) for s in sensors], np.float32)
    cells_n = size * size
    for order in (ROW, COL):
        for max_cells in (0, 64):
            dst = Dest(2, cells_n + 1)
            rc = raw_visibility(seg, 2, dst, origins, points=pts.data_ptr(), stride=stride, n_points=n_pts, labels=d_labels.data_ptr(), max_cells=max_cells, order=order)
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
            torch.cuda.synchronize()
            host = dst.host()
            for i in range(2):
                want = visibility_ref.expected_visibility(*truth[i], max_cells, ORDER[order])
                assert want[1][0] > 3000
                check_cloud(host, i, want, size, size, cells_n + 1, f"148 {ORDER[order]} R={max_cells} cloud {i}")
    seg.close()


SCAN = dict(min_points=2, lo=0.3, hi=2.5)


@pytest.fixture(scope="module")
def scan_scene():
    """one 64-ring scan on a 364 x 364 map that an earlier scan warmed, the labels the batch gave it (held to be the oracle's), and the
    oracle's truth"""
    import torch

    length, res = GEOMETRY[364]
    seg = api.GroundSegmentation().init(length, res, n_slots=3, max_points=20000)
    seg.reset_maps(odom_z=0.2)
    ref = oracle.OracleMap(length, res, odom_z=0.2)
    clouds = [synth.hdl64_cloud(seed=7500, n_az=280), synth.hdl64_cloud(seed=7501, n_az=300)]
    stride = stride_of(clouds)
    origin = np.array([[0.4, -0.3, 1.7]], np.float32)
    outs = []
    for c in clouds:
        pts = batch_points([c], stride)
        outs.append((pts, seg.filter_batch(pts, [len(c)], origin, np.full(1, -1.73), slots=[1], want_masks=True)))
        want_labels = ref.filter_cloud(c, tuple(float(v) for v in origin[0]), -1.73)["label"]
    torch.cuda.synchronize()
    pts, out = outs[-1]
    cloud = clouds[-1]
    assert np.array_equal(out.labels.cpu().numpy()[0, : len(cloud)], want_labels), "the batch's labels are not the oracle's"
    truth = visibility_ref.cloud_truth(ref, cloud, want_labels, origin[0], SCAN["min_points"], SCAN["lo"], SCAN["hi"])
    assert truth[2] is not None and int(truth[0].sum()) > 100 and int(truth[1].sum()) > 3000
    yield dict(seg=seg, pts=pts, out=out, n=len(cloud), stride=stride, origin=origin, truth=truth)
    seg.close()


@pytest.mark.parametrize("order", [ROW, COL])
def test_a_real_scan(scan_scene, order):
    import torch

    sc = scan_scene
    seg = sc["seg"]
    want = visibility_ref.expected_visibility(*sc["truth"], 0, ORDER[order])
    assert want[1][0] > 10000 and want[1][1] > 10000 and want[1][2] > 100
    plane_stride = seg.rows * seg.cols + 3
    dst = Dest(1, plane_stride)
    which = dict(labels=sc["out"].labels.data_ptr()) if order == ROW else dict(masks=sc["out"].label_masks.data_ptr())
    rc = raw_visibility(seg, 1, dst, sc["origin"], first_slot=1, points=sc["pts"].data_ptr(), stride=sc["stride"], n_points=[sc["n"]], min_points=SCAN["min_points"],
                        lo=SCAN["lo"], hi=SCAN["hi"], order=order, **which)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    check_cloud(dst.host(), 0, want, 364, 364, plane_stride, f"a real scan, {ORDER[order]}")


def test_agreement_with_cluster_clouds(scan_scene):
    import torch

    sc = scan_scene
    seg = sc["seg"]
    kw = dict(slots=[1], min_points=SCAN["min_points"], min_height=SCAN["lo"], max_height=SCAN["hi"])
    for order, which in (("row", dict(labels=sc["out"].labels)), ("col", dict(masks=sc["out"].label_masks))):
        vis = seg.visibility_clouds(sc["pts"], [sc["n"]], sc["origin"], order=order, **kw, **which)
        clusters = seg.cluster_clouds(sc["pts"], [sc["n"]], order=order, max_clusters=0, point_clusters=False, **kw, **which)
        torch.cuda.synchronize()
        state, ids = vis.state.cpu().numpy(), clusters.cell_cluster.cpu().numpy()
        assert np.array_equal(state == OCCUPIED, ids >= 0) and int((ids >= 0).sum()) == int(vis.counts[0, 2].item()) > 100
        assert set(np.unique(state).tolist()) == {FREE, UNKNOWN, OCCUPIED}


def test_a_map_of_a_million_cells():
    """1000 x 1000: the bitmap of the map is 125 000 bytes of a work-group's local memory; a few hundred returns on the border and the sensor
    in the middle, in a corner and on a border: the rays cross the whole map"""
    import torch

    size = 1000
    seg = api.GroundSegmentation().init(330.0, 0.33, n_slots=3, max_points=1024)
    assert seg.rows == seg.cols == size
    seg.reset_maps(odom_z=ODOM_Z)
    ref = oracle.OracleMap(330.0, 0.33, odom_z=ODOM_Z)
    rng = np.random.default_rng(7600)
    sensors = [(500, 500), (0, 999), (999, 123)]
    clouds, labels, truth = [], [], []
    for k in range(3):
        along = rng.choice(size, 70, replace=False)
        cells = np.concatenate([np.stack([np.zeros(70, np.int64), along], 1), np.stack([np.full(70, 999), along], 1), np.stack([along, np.zeros(70, np.int64)], 1),
                                np.stack([along, np.full(70, 999)], 1), [[0, 0], [999, 999], [0, 999], [999, 0], [499, 501], [250, 750]]])
        cells = np.unique(cells, axis=0)
        lab = rng.choice(np.array([49, 99], np.uint8), len(cells))
        x, y = cell_centres(ref, cells)
        clouds.append(cloud_of(x, y, np.full(len(cells), 0.7, np.float32)))
        labels.append(lab)
        occupied, hit = np.zeros((size, size), bool), np.zeros((size, size), bool)
        hit[cells[:, 0], cells[:, 1]] = True
        occupied[cells[lab == 99, 0], cells[lab == 99, 1]] = True
        truth.append((occupied, hit, sensors[k]))
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    assert min(n_pts) > 250
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    host_labels = np.zeros((3, stride), np.uint8)
    for i, lab in enumerate(labels):
        host_labels[i, : len(lab)] = lab
    d_labels = torch.from_numpy(host_labels).cuda()
    origins = np.array([sensor_xy(ref, s) for s in sensors], np.float32)
    cells_n = size * size
    dst = Dest(3, cells_n + 5)
    rc = raw_visibility(seg, 3, dst, origins, slots=[2, 0, 1], points=pts.data_ptr(), stride=stride, n_points=n_pts, labels=d_labels.data_ptr(), order=COL)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    for i in range(3):
        want = visibility_ref.expected_visibility(*truth[i], 0, "col")
        assert want[1][0] > 50000
        check_cloud(host, i, want, size, size, cells_n + 5, f"1000 x 1000, cloud {i}")
    seg.close()


# ---------------------------------------------------------------- 4. chaining into the clearance

def test_state_planes_are_seed_planes_of_the_clearance(pattern_scene):
    import torch

    sc = pattern_scene
    seg, names = sc["seg"], sc["names"]
    pick = [names.index(k) for k in ("random", "ring", "through_occupied", "empty")]
    vis = seg.visibility_clouds(sc["pts"][pick].contiguous(), [sc["n_pts"][i] for i in pick], sc["origins"][pick], labels=sc["labels"][pick].contiguous(),
                                slots=[sc["slots"][i] for i in pick], min_points=2)
    field = seg.clearance_planes(vis.state)
    torch.cuda.synchronize()
    want = sc["expected"](0, ROW)
    state = vis.state.cpu().numpy()
    for j, i in enumerate(pick):
        assert np.array_equal(state[j], want[i][0]), names[i]
        dist2, nearest, distance, n_seeds = clearance_ref.expected_clearance(state[j] >= 0, 0, "row", np.float32(seg.resolution))
        assert n_seeds == int(want[i][1][1] + want[i][1][2]) == int(field.n_occupied[j].item())  # unknown and occupied cells
        assert np.array_equal(field.dist2[j].cpu().numpy(), dist2) and np.array_equal(field.nearest[j].cpu().numpy(), nearest), names[i]
        assert np.array_equal(field.distance[j].cpu().numpy().view(np.uint32), distance), names[i]


# ---------------------------------------------------------------- 5. right behind a batch, on the same stream, labels from its masks

def test_right_behind_a_batch_on_the_same_stream():
    import torch

    slots = [2, 0, 3]
    K = len(slots)
    length, res = GEOMETRY[79]
    clouds = [synth.hdl64_cloud(seed=7700 + k, n_az=90 + 10 * k) for k in range(K)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    seg = api.GroundSegmentation().init(length, res, n_slots=4, max_points=stride)
    pts = batch_points(clouds, stride)
    origins, base_z = np.array([[0.0, 0.0, 0.0], [3.0, -2.0, 0.0], [-4.5, 4.5, 0.0]], np.float32), np.full(K, -1.73)
    plane_stride = seg.rows * seg.cols + 1
    dst = Dest(K, plane_stride)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(odom_z=0.0, on_torch_stream=True)
        out = seg.filter_batch(pts, n_pts, origins, base_z, slots=slots, want_masks=True)
        rc = raw_visibility(seg, K, dst, origins, slots=slots, points=pts.data_ptr(), stride=stride, n_points=n_pts, masks=out.label_masks.data_ptr(), lo=0.2, hi=3.0)
        assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    free = 0
    for i in range(K):
        ref = oracle.OracleMap(length, res)
        lab = ref.filter_cloud(clouds[i], tuple(float(v) for v in origins[i]), -1.73)["label"]
        truth = visibility_ref.cloud_truth(ref, clouds[i], lab, origins[i], 1, 0.2, 3.0)
        assert truth[2] is not None
        want = visibility_ref.expected_visibility(*truth, 0, "row")
        free += int(want[1][0])
        check_cloud(host, i, want, seg.rows, seg.cols, plane_stride, f"behind the batch, cloud {i}")
    assert free >= 1000, free
    seg.close()


# ---------------------------------------------------------------- 6. past the ring

def test_past_the_ring_back_to_back(pattern_scene):
    """PARAM_RING + 2 calls on one caller stream without a synchronisation, every one with other clouds, slot lists, radii and orders"""
    import torch

    sc = pattern_scene
    seg, names = sc["seg"], sc["names"]
    n = len(names)
    picks = [[0, 1, 2, 16], [3, 4, 5], [17, 0], [14], [6, 7, 8, 9, 15], [10, 11, 12, 13, 18, 19]][: PARAM_RING + 2]
    assert len(picks) == PARAM_RING + 2 and max(max(p) for p in picks) < n
    cells = 79 * 79
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    calls = []
    with torch.cuda.stream(stream):
        for k, pick in enumerate(picks):
            order, max_cells = (ROW, COL)[k % 2], (0, 7, 200)[k % 3]
            dst = Dest(len(pick), cells + 3)
            rc, keep = pattern_call(sc, dst, pick, max_cells=max_cells, order=order)
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
            calls.append((pick, order, max_cells, dst, keep))
    torch.cuda.synchronize()
    for k, (pick, order, max_cells, dst, _) in enumerate(calls):
        host, want = dst.host(), sc["expected"](max_cells, order)
        for j, i in enumerate(pick):
            check_cloud(host, j, want[i], 79, 79, cells + 3, f"call {k}, {names[i]}")


# ---------------------------------------------------------------- 7. nothing else changes

def test_nothing_changes():
    import torch

    slots = [4, 1, 5, 2]
    K = len(slots)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000) for _ in range(2)]
    base = [synth.hdl64_cloud(seed=7800 + k, n_az=150 + 7 * k) for k in range(K)]
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
        if which == 0:  # the call between the two batches: on every map of the context (two of them fresh), and of the batch
            all_pts = torch.zeros((6, stride, 16), dtype=torch.uint8, device="cuda")  # (every point at the origin, z = 0: h = -0.1 on a fresh map)
            all_labels = torch.full((6, stride), 99, dtype=torch.uint8, device="cuda")
            far = np.tile(np.array([[10.0, -7.0, 0.0]], np.float32), (6, 1))
            every = seg.visibility_clouds(all_pts, [stride] * 6, far, labels=all_labels, slots=list(range(6)), min_height=-100.0, max_height=100.0)
            banded = seg.visibility_clouds(all_pts, [stride] * 6, far, labels=all_labels, slots=list(range(6)), min_height=-0.15, max_height=-0.05, counts=False)
            seen = seg.visibility_clouds(pts[0], n_pts[0], origins, masks=first.label_masks, slots=slots, min_points=2, min_height=0.3, max_height=2.5, max_cells=40)
        # the lazily kept layers are still pending behind the calls: their first reader computes them, to the values of the twin
        assert lazy_count(seg) == K
        pending = seg.export_layers(lazy, slots=slots)
        assert lazy_count(seg) == 0
        second = seg.filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
        planes = seg.export_layers()
        torch.cuda.synchronize()
        if which == 0:  # one cell per map holds all the points, and one ray leads to it: 10 / 0.33 = 30 cells and 7 / 0.33 = 21
            got = every.counts.cpu().numpy()
            assert np.array_equal(got[:, 2], np.ones(6, np.int32)) and np.all(got[:, 0] == got[0, 0]) and 30 <= got[0, 0] <= 31 and np.all(got.sum(axis=1) == 364 * 364)
            occupied = (banded.state == OCCUPIED).sum(dim=(1, 2)).cpu().numpy()  # on the two fresh maps (0 and 3) the band admits exactly h = 0 - odom_z
            assert occupied[0] == occupied[3] == 1, occupied
            assert int(seen.counts[:, 0].min().item()) > 1000 and int(seen.counts[:, 2].min().item()) > 0
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


# ---------------------------------------------------------------- 8. twice the same

def test_twice_the_same(pattern_scene, scan_scene):
    import torch

    sc, scan = pattern_scene, scan_scene
    n, cells = len(sc["names"]), 79 * 79
    runs = []
    for _ in range(2):
        a, b = Dest(n, cells + 3), Dest(1, 364 * 364)
        rc, keep = pattern_call(sc, a, max_cells=11, order=COL)
        assert rc == 0
        assert raw_visibility(scan["seg"], 1, b, scan["origin"], first_slot=1, points=scan["pts"].data_ptr(), stride=scan["stride"], n_points=[scan["n"]],
                              labels=scan["out"].labels.data_ptr(), min_points=2, lo=0.3, hi=2.5) == 0
        runs.append((a, b))
    torch.cuda.synchronize()
    for first, second in zip(runs[0], runs[1]):
        x, y = first.host(), second.host()
        for key in x:
            assert np.array_equal(x[key], y[key]), f"{key} differs between two runs"
    assert int(runs[0][1].host()["counts"][0, 0]) > 10000


# ---------------------------------------------------------------- 9. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=4096)
    seg.reset_maps(odom_z=0.4)
    clouds = [synth.hdl64_cloud(seed=7900 + k, n_az=40) for k in range(2)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    assert stride <= 4096
    warm_maps(seg, [4, 1], seed=7910, frames=1, n_az=40)
    before = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    labels = torch.full((2, stride), 99, dtype=torch.uint8, device="cuda")
    cells = seg.rows * seg.cols
    dst = Dest(2, cells)
    P, Lb = pts.data_ptr(), labels.data_ptr()
    zero = np.zeros((2, 3), np.float32)

    def call(n=2, origins=zero, slots=None, first=0, fmt=_lib.GG_POINT16, points=P, stride=stride, n_points=n_pts, labels=Lb, masks=0, **kw):
        return raw_visibility(seg, n, dst, origins, slots=slots, first_slot=first, fmt=fmt, points=points, stride=stride, n_points=n_points, labels=labels, masks=masks, **kw)

    x = _lib.GGCloudVisibility()
    x.n = 2
    assert seg._L.gg_visibility_clouds(None, C.byref(x), None) == INVALID
    assert seg._L.gg_visibility_clouds(seg._ctx, None, None) == INVALID
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
    assert call(origins=None) == INVALID
    assert call(state=0) == INVALID
    assert call(plane_stride=cells - 1) == INVALID
    assert call(order=2) == INVALID
    assert call(order=-1) == INVALID
    assert call(max_cells=-1) == INVALID
    assert call(min_points=0) == INVALID
    assert call(min_points=-3) == INVALID
    assert call(lo=math.nan) == INVALID
    assert call(hi=math.nan) == INVALID
    assert call(n=0, origins=None, points=0, n_points=None, labels=0, fmt=9, stride=10 ** 9, state=0, counts=0, min_points=-1, order=7, plane_stride=0, max_cells=-4,
                lo=math.nan) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel()
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    assert same_bits(before.cpu().numpy(), after.cpu().numpy())
    assert call(slots=[4, 1]) == 0, seg._L.gg_last_error(seg._ctx)  # ... and the same arguments without a mistake are accepted
    torch.cuda.synchronize()
    host = dst.host()
    assert fresh_count(seg) == fresh_before
    for i in range(2):
        counts = host["counts"][i].view(np.int32)
        assert int(counts.sum()) == cells and counts[0] > 0 and counts[2] > 0
        state = host["state"][i * cells: (i + 1) * cells].view(np.int32)
        assert [int((state == v).sum()) for v in (FREE, UNKNOWN, OCCUPIED)] == counts.tolist()
    seg.close()


# ---------------------------------------------------------------- 10. the Python entry point

def test_python_entry_point(pattern_scene):
    import torch

    sc = pattern_scene
    seg, n, slots, names = sc["seg"], len(sc["slots"]), sc["slots"], sc["names"]
    args = (sc["pts"], sc["n_pts"], sc["origins"])
    a = seg.visibility_clouds(*args, labels=sc["labels"], slots=slots, min_points=2)
    assert isinstance(a, api.VisibilityOutputs)
    for t, shape in ((a.state, (n, 79, 79)), (a.counts, (n, 3))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    masks = torch.from_numpy(masks_of(sc["host_labels"], sc["stride"])).cuda()
    b = seg.visibility_clouds(sc["pts"], sc["n_pts"], sc["origins"].tolist(), masks=masks, slots=slots, min_points=2, order="col", max_cells=7, counts=False)
    assert tuple(b.state.shape) == (n, 79, 79) and b.counts is None
    b.state.fill_(SIGNED_SENTINEL)
    again = seg.visibility_clouds(*args, masks=masks, slots=slots, min_points=2, order="col", max_cells=7, counts=False, out=b)
    assert again is b
    own = seg.visibility_clouds(*args, labels=sc["labels"], slots=slots, min_points=2, max_cells=200, on_torch_stream=False)
    with pytest.raises(ValueError):
        seg.visibility_clouds(*args, slots=slots)
    with pytest.raises(ValueError):
        seg.visibility_clouds(*args, labels=sc["labels"], masks=masks, slots=slots)
    with pytest.raises(ValueError):
        seg.visibility_clouds(sc["pts"], sc["n_pts"], sc["origins"][:, :2], labels=sc["labels"], slots=slots)
    with pytest.raises(ValueError):
        seg.visibility_clouds(*args, labels=sc["labels"], slots=slots, order="fortran")
    with pytest.raises(ValueError):
        seg.visibility_clouds(*args, labels=sc["labels"], slots=slots, out=api.VisibilityOutputs(state=torch.empty((n, 79, 80), dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError):
        seg.visibility_clouds(*args, labels=sc["labels"], slots=slots, out=api.VisibilityOutputs(state=torch.empty((n, 79, 79), dtype=torch.int64, device="cuda")))
    with pytest.raises(ValueError):
        seg.visibility_clouds(*args, labels=sc["labels"], slots=slots, counts=False, out=a)  # (counts that are not asked for)
    torch.cuda.synchronize()
    seg.synchronize()
    want, want7c, want200 = sc["expected"](0, ROW), sc["expected"](7, COL), sc["expected"](200, ROW)
    for i in range(n):
        assert np.array_equal(a.state[i].cpu().numpy(), want[i][0]) and np.array_equal(a.counts[i].cpu().numpy(), want[i][1]), names[i]
        assert np.array_equal(b.state[i].cpu().numpy(), want7c[i][0]), names[i]
        assert np.array_equal(own.state[i].cpu().numpy(), want200[i][0]) and np.array_equal(own.counts[i].cpu().numpy(), want200[i][1]), names[i]
