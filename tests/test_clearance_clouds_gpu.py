"""gg_clearance_clouds (the exact squared Euclidean distance of every cell to the nearest occupied cell, which cell that is and the distance
in metres, of many maps in device memory, one call) on the device.  Expected values come from numpy alone (tests/clearance_ref.py: a brute
force over the occupied cells, itself held against scipy.ndimage.distance_transform_edt by tests/test_clearance_clouds_cpu.py) on an
occupancy that is a pattern (seed mode) or the CPU oracle's (cloud mode: tests/test_cluster_clouds_gpu.expectation).  Every comparison is on
bits; there is no tolerance.

A non-square map cannot be made: gg_geometry has ONE length, so every map of this library is square.  The shape case that would be
non-square runs at 148 x 148, a side that is no multiple of 64 and none of the other tests' sizes."""
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
from tests import clearance_ref  # noqa: E402
from tests.test_cluster_clouds_gpu import Dest as ClusterDest, cell_centres, cloud_of, expectation, raw_cluster, small_chunk_context  # noqa: E402
from tests.test_export_layers_gpu import SENTINEL, batch_points, fresh_count, same_bits, stride_of, warm_maps  # noqa: E402
from tests.test_split_clouds_gpu import GEOMETRY, PARAM_RING, lazy_count, masks_of, points_tensor, transform_of  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
SIGNED_SENTINEL = SENTINEL - (1 << 32) if SENTINEL >= (1 << 31) else SENTINEL
INF = math.inf
NONE = clearance_ref.NONE
assert NONE == _lib.GG_CLEARANCE_NONE


# ---------------------------------------------------------------- helpers

class Dest:
    """sentinel-filled destinations of one call: per kind n planes plane_stride words apart (and `slack` words behind), and the counts"""

    def __init__(self, n, plane_stride, slack=0):
        import torch

        def filled(words):
            return torch.full((max(words, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

        self.n, self.plane_stride = n, plane_stride
        self.dist2, self.nearest, self.distance, self.counts = (filled(n * plane_stride + slack), filled(n * plane_stride + slack),
                                                                filled(n * plane_stride + slack), filled(n))

    def host(self):
        return {k: getattr(self, k).cpu().numpy().view(np.uint32) for k in ("dist2", "nearest", "distance", "counts")}

    def all_sentinel(self):
        return all(bool((t == SIGNED_SENTINEL).all().item()) for t in (self.dist2, self.nearest, self.distance, self.counts))


def raw_clearance(seg, n, dest, seeds=0, seed_stride=0, slots=None, first_slot=0, fmt=_lib.GG_POINT16, points=0, stride=0, n_points=None, labels=0,
                  masks=0, transforms=None, min_points=1, lo=-INF, hi=INF, max_cells=0, order=ROW, stream=None, own=False, **over):
    """gg_clearance_clouds as the C ABI has it (device addresses as integers, 0 = null); returns the status.  `over`: dist2, plane_stride,
    nearest, distance, counts in place of what `dest` gives"""
    import torch

    x = _lib.GGCloudClearance()
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
    x.d_seeds, x.seed_stride, x.max_cells, x.order = seeds or None, seed_stride, max_cells, order
    x.d_dist2 = over.get("dist2", dest.dist2.data_ptr()) or None
    x.plane_stride = over.get("plane_stride", dest.plane_stride)
    x.d_nearest = over.get("nearest", dest.nearest.data_ptr()) or None
    x.d_distance = over.get("distance", dest.distance.data_ptr()) or None
    x.d_n_occupied = over.get("counts", dest.counts.data_ptr()) or None
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_clearance_clouds(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def derive(free, rows, cols, max_cells, order):
    """clearance_ref.expected_clearance(occ, max_cells, order) from free = expected_clearance(occ, 0, "row"), which took the brute force:
    beyond the radius there is no obstacle (tests/test_clearance_clouds_cpu.py holds this against the brute force itself), and a cell's index
    in the other order is arithmetic"""
    dist2, nearest, distance, n_occ = (np.array(v) for v in free)
    if max_cells > 0:
        far = dist2.astype(np.int64) > max_cells * max_cells
        dist2[far], nearest[far], distance[far] = NONE, -1, clearance_ref.INF_BITS
    if order == "col":
        nearest = np.where(nearest < 0, -1, nearest // cols + (nearest % cols) * rows).astype(np.int32)
    return dist2, nearest, distance, int(n_occ)


def check_map(host, i, want, order, rows, cols, plane_stride, tag, given=("nearest", "distance", "counts")):
    """map i of a downloaded Dest against an expectation: the three planes and the count, the words behind every plane, and the elements of
    an output that was not handed over"""
    at = i * plane_stride
    for key, plane in (("dist2", want[0]), ("nearest", want[1]), ("distance", want[2])):
        words = host[key][at: at + plane_stride]
        if key != "dist2" and key not in given:
            assert np.all(words == SENTINEL), f"{tag}: map {i}: {key} was not handed over and was written"
            continue
        got = words[: rows * cols]
        got = got.reshape(rows, cols) if order == ROW else got.reshape((rows, cols), order="F")
        bad = np.argwhere(got != np.asarray(plane).view(np.uint32))
        assert len(bad) == 0, f"{tag}: map {i}: {len(bad)} cells of {key} differ, first {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {np.asarray(plane).view(np.uint32)[tuple(bad[0])]:#x}"
        assert np.all(words[rows * cols:] == SENTINEL), f"{tag}: map {i}: the words behind the {key} plane were written"
    if "counts" in given:
        assert int(host["counts"][i]) == want[3], f"{tag}: map {i}: n_occupied {int(host['counts'][i])} != {want[3]}"
    else:
        assert host["counts"][i] == SENTINEL, f"{tag}: map {i}: n_occupied was not handed over and was written"


def seed_planes(occupancies, order, seed_stride, rng):
    """the seed planes of boolean occupancies, laid out as `order` says, seed_stride words apart: occupied words are >= 0 (0, a cluster id,
    the largest int32), the others negative (-1, a small negative, the smallest int32)"""
    import torch

    n = len(occupancies)
    host = np.full(n * seed_stride, -1, dtype=np.int32)
    for i, occ in enumerate(occupancies):
        yes = rng.choice(np.array([0, 0, 5, 4711, 0x7FFFFFFF], dtype=np.int64), size=occ.shape)
        no = rng.choice(np.array([-1, -1, -7, -0x80000000], dtype=np.int64), size=occ.shape)
        host[i * seed_stride: i * seed_stride + occ.size] = clearance_ref.as_plane(np.where(occ, yes, no).astype(np.int32), ORDER[order]).reshape(-1)
    return torch.from_numpy(host).cuda()


def plain_context(size, n_slots, max_points=1024):
    length, res = {**GEOMETRY, 148: (49.0, 0.33)}[size]
    seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=max_points)
    assert seg.rows == seg.cols == size
    return seg


# ---------------------------------------------------------------- 1. seed mode, every pattern

@pytest.fixture(scope="module")
def pattern_reference():
    """every pattern of clearance_ref.patterns(79, 79) with its unbounded row-major expectation -- the brute force, once"""
    pats = clearance_ref.patterns(79, 79)
    assert len(pats) == 21
    return pats, {name: clearance_ref.expected_clearance(occ, 0, "row", np.float32(0.33)) for name, occ in pats.items()}


@pytest.fixture(scope="module")
def seed_context():
    seg = plain_context(79, 24)
    assert np.float32(seg.resolution) == np.float32(0.33)
    yield seg
    seg.close()


@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("max_cells", [0, 1, 7, 200])
def test_seed_mode_patterns(pattern_reference, seed_context, max_cells, order):
    import torch

    pats, free = pattern_reference
    seg, names = seed_context, list(pats)
    n, cells = len(names), seg.rows * seg.cols
    plane_stride, seed_stride = cells + 3, cells + 5
    seeds = seed_planes([pats[k] for k in names], order, seed_stride, np.random.default_rng(6100))
    dst = Dest(n, plane_stride, slack=129)
    fresh_before = fresh_count(seg)
    rc = raw_clearance(seg, n, dst, seeds=seeds.data_ptr(), seed_stride=seed_stride, max_cells=max_cells, order=order,
                       fmt=77, stride=10 ** 9, first_slot=-3, min_points=-1, lo=math.nan)  # (ignored in seed mode)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    host = dst.host()
    for key in ("dist2", "nearest", "distance"):
        assert np.all(host[key][n * plane_stride:] == SENTINEL)
    for i, name in enumerate(names):
        check_map(host, i, derive(free[name], 79, 79, max_cells, ORDER[order]), order, 79, 79, plane_stride, f"{name} R={max_cells} {ORDER[order]}")
    four = host["nearest"][names.index("four_corners") * plane_stride:][39 * 79 + 39]
    assert four == (0 if max_cells in (0, 200) else 0xFFFFFFFF)  # the four-way tie goes to (0, 0); 2 * 39^2 lies beyond 7 cells


def test_seed_mode_absent_outputs(pattern_reference, seed_context):
    import torch

    pats, free = pattern_reference
    seg, cells = seed_context, 79 * 79
    names = ["random_30", "empty", "pairs"]
    seeds = seed_planes([pats[k] for k in names], ROW, cells, np.random.default_rng(6110))
    for given in ((), ("nearest",), ("distance", "counts")):
        dst = Dest(3, cells)
        rc = raw_clearance(seg, 3, dst, seeds=seeds.data_ptr(), seed_stride=cells, **{k: 0 for k in ("nearest", "distance", "counts") if k not in given})
        assert rc == 0, seg._L.gg_last_error(seg._ctx)
        torch.cuda.synchronize()
        host = dst.host()
        for i, name in enumerate(names):
            check_map(host, i, free[name], ROW, 79, 79, cells, f"{name} given {given}", given=given)


# ---------------------------------------------------------------- 2. cloud mode

ODOM_Z = 0.2
BAND = (0.25, 1.5)  # on h = z - ODOM_Z
CLOUD_PATTERNS = ["random_30", "pairs", "empty", "spiral", "four_corners", "borders"]
CLOUD_SLOTS = [5, 2, 7, 0, 6, 3]


def pattern_cloud(ref, occ, rng):
    """(cloud in the map frame, label bytes) that realise `occ` under min_points = 2 and BAND on a fresh map of ground ODOM_Z: two points
    inside the band in every occupied cell, and in free cells points that do not make them occupied -- one point inside the band, two whose
    z lies inside the band but whose height z - ODOM_Z lies below it (a ground of 0 instead of the fresh map's constant would admit them),
    two above it, two NaN-free points of other labels -- in no particular order"""
    lo, hi = BAND
    inside = [np.float32(ODOM_Z + lo + 0.05), np.float32(ODOM_Z + hi - 0.1), np.float32(ODOM_Z + 0.7)]
    below = np.float32(lo + 0.5 * ODOM_Z)
    assert below > lo and below - np.float32(ODOM_Z) < lo
    cells, z, lab = [], [], []
    for r, c in np.argwhere(occ):
        k = 2 + int(rng.integers(0, 2))
        cells += [(r, c)] * k
        z += [inside[int(v)] for v in rng.integers(0, 3, 2)] + [np.float32(ODOM_Z + hi + 1.0)] * (k - 2)
        lab += [99] * k
    free = np.argwhere(~occ)
    for r, c in free[rng.permutation(len(free))[: min(len(free), 300)]]:
        kind = int(rng.integers(0, 4))
        zs, ls = [([inside[0]], [99]), ([below, below], [99, 99]), ([np.float32(9.0)] * 2, [99, 99]), ([inside[2]] * 2, [49, 7])][kind]
        cells += [(r, c)] * len(zs)
        z += zs
        lab += ls
    if not cells:
        return synth.empty_cloud(0), np.zeros(0, np.uint8)
    perm = rng.permutation(len(cells))
    x, y = cell_centres(ref, np.array(cells)[perm])
    return cloud_of(x, y, np.array(z, np.float32)[perm]), np.array(lab, np.uint8)[perm]


@pytest.fixture(scope="module")
def cloud_scene(pattern_reference):
    """one crafted cloud per pattern of CLOUD_PATTERNS on fresh maps of a GG_PW=128 context, through a permuted slot list; per use_tf the
    clouds as the caller gives them (the sensor frame, brought to the map by transform_of()) and the oracle's occupancy, made once"""
    pats, free = pattern_reference
    length, res = GEOMETRY[79]
    ref = oracle.OracleMap(length, res, odom_z=ODOM_Z)
    rng = np.random.default_rng(6200)
    made = [pattern_cloud(ref, pats[name], rng) for name in CLOUD_PATTERNS]
    map_clouds, labels = [m[0] for m in made], [m[1] for m in made]
    n_pts = [len(c) for c in map_clouds]
    assert n_pts[CLOUD_PATTERNS.index("empty")] > 0 and n_pts[CLOUD_PATTERNS.index("spiral")] > 6400  # (more than 50 chunks of 128 points)
    n_pts[CLOUD_PATTERNS.index("four_corners")] = 0  # this cloud is handed over with n_points = 0: its map is empty
    stride = stride_of(map_clouds)
    seg = small_chunk_context(8, stride)
    seg.reset_maps(odom_z=ODOM_Z)
    R, t, tf = transform_of()
    cache = {}

    def variant(use_tf):
        if use_tf not in cache:
            given = map_clouds
            if use_tf:  # the sensor-frame clouds whose transform lands in the same cells (half a cell of margin against the rounding)
                given = []
                for c in map_clouds:
                    s = c.copy()
                    if len(c):
                        p = (np.stack([c["x"], c["y"], c["z"]], axis=1).astype(np.float64) - t) @ R
                        s["x"], s["y"], s["z"] = p[:, 0].astype(np.float32), p[:, 1].astype(np.float32), p[:, 2].astype(np.float32)
                    given.append(s)
            in_map = [kitti.transform_cloud(c, R, t) if use_tf and len(c) else c for c in given]
            want = []
            for i, name in enumerate(CLOUD_PATTERNS):
                plane = expectation(ref, in_map[i][: n_pts[i]], labels[i], 2, BAND[0], BAND[1], 8, "row", ground=ODOM_Z)[0]
                occ = plane >= 0
                if not use_tf:  # (with the transform the heights carry its rounding: a point on a bound of the band may fall either way)
                    assert np.array_equal(occ, pats[name] if n_pts[i] else np.zeros_like(occ)), name
                want.append((occ, clearance_ref.expected_clearance(occ, 0, "row", np.float32(seg.resolution))))
            cache[use_tf] = dict(given=given, want=want, tf=[tf] * len(given) if use_tf else None)
        return cache[use_tf]

    host_labels = np.zeros((len(made), stride), np.uint8)
    for i, lab in enumerate(labels):
        host_labels[i, : len(lab)] = lab
    yield dict(seg=seg, variant=variant, n_pts=n_pts, stride=stride, labels=host_labels)
    seg.close()


@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("use_masks", [False, True])
@pytest.mark.parametrize("fmt", [_lib.GG_POINT16, _lib.GG_POINT32])
def test_cloud_mode(cloud_scene, fmt, use_masks, use_tf):
    import torch

    sc, v = cloud_scene, cloud_scene["variant"](use_tf)
    seg, n, stride, n_pts = sc["seg"], len(CLOUD_PATTERNS), sc["stride"], sc["n_pts"]
    order = COL if use_masks else ROW
    max_cells = 9 if fmt == _lib.GG_POINT32 else 0
    pts = points_tensor(v["given"], stride, fmt)
    lab = torch.from_numpy(masks_of(sc["labels"], stride) if use_masks else sc["labels"]).cuda()
    which = dict(masks=lab.data_ptr()) if use_masks else dict(labels=lab.data_ptr())
    cells = seg.rows * seg.cols
    plane_stride = cells + 3
    dst, again = Dest(n, plane_stride), Dest(n, plane_stride)
    assert fresh_count(seg) == 8
    common = dict(slots=CLOUD_SLOTS, fmt=fmt, points=pts.data_ptr(), stride=stride, n_points=n_pts, transforms=v["tf"], min_points=2, lo=BAND[0], hi=BAND[1])
    rc = raw_clearance(seg, n, dst, max_cells=max_cells, order=order, **common, **which)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    # the same field from the id planes gg_cluster_clouds gives for the same arguments, handed over as seeds
    clusters = ClusterDest(n, cells + 1, stride, 0)
    rc = raw_cluster(seg, n, CLOUD_SLOTS, 0, fmt, pts.data_ptr(), stride, n_pts, clusters, transforms=v["tf"], min_points=2, lo=BAND[0], hi=BAND[1],
                     conn=8, order=order, ids=0, **which)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    rc = raw_clearance(seg, n, again, seeds=clusters.planes.data_ptr(), seed_stride=cells + 1, max_cells=max_cells, order=order)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == 8
    host, host2 = dst.host(), again.host()
    tag = f"{'point16' if fmt else 'point32'} {'masks' if use_masks else 'labels'} {'tf' if use_tf else 'map frame'} {ORDER[order]}"
    for i, name in enumerate(CLOUD_PATTERNS):
        want = derive(v["want"][i][1], 79, 79, max_cells, ORDER[order])
        check_map(host, i, want, order, 79, 79, plane_stride, f"{tag} {name}")
    for key in host:
        assert np.array_equal(host[key], host2[key]), f"{tag}: {key} differs between the cloud mode and the seed mode on gg_cluster_clouds' planes"
    assert int(host["counts"][CLOUD_PATTERNS.index("four_corners")]) == 0 and int(host["counts"][CLOUD_PATTERNS.index("spiral")]) > 3000


# ---------------------------------------------------------------- 3. shapes

def test_a_side_that_is_no_multiple_of_64():
    import torch

    size = 148
    seg = plain_context(size, 3)
    rng = np.random.default_rng(6300)
    occs = [rng.random((size, size)) < 0.002, rng.random((size, size)) < 0.2, np.zeros((size, size), bool)]
    occs[2][147, 0] = occs[2][0, 147] = occs[2][77, 64] = True
    want = [clearance_ref.expected_clearance(o, 0, "row", np.float32(seg.resolution)) for o in occs]
    cells = size * size
    for order in (ROW, COL):
        for max_cells in (0, 64):
            dst = Dest(3, cells + 1)
            seeds = seed_planes(occs, order, cells + 7, rng)
            assert raw_clearance(seg, 3, dst, seeds=seeds.data_ptr(), seed_stride=cells + 7, max_cells=max_cells, order=order) == 0, seg._L.gg_last_error(seg._ctx)
            torch.cuda.synchronize()
            host = dst.host()
            for i in range(3):
                check_map(host, i, derive(want[i], size, size, max_cells, ORDER[order]), order, size, size, cells + 1, f"148 {ORDER[order]} R={max_cells} map {i}")
    seg.close()


@pytest.fixture(scope="module")
def headline_context():
    seg = plain_context(364, 2)
    yield seg
    seg.close()


@pytest.mark.parametrize("order", [ROW, COL])
def test_headline_map_with_150_cells(headline_context, order):
    import torch

    seg, size = headline_context, 364
    rng = np.random.default_rng(6310)
    occ = np.zeros((size, size), bool)
    occ.reshape(-1)[rng.choice(size * size, 150, replace=False)] = True
    want = clearance_ref.expected_clearance(occ, 0, ORDER[order], np.float32(seg.resolution))
    assert want[3] == 150 and int(want[0].max()) > 40 * 40
    cells = size * size
    dst = Dest(1, cells + 3)
    seeds = seed_planes([occ], order, cells, rng)
    assert raw_clearance(seg, 1, dst, seeds=seeds.data_ptr(), seed_stride=cells, order=order, first_slot=1) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    check_map(dst.host(), 0, want, order, size, size, cells + 3, f"364, 150 cells, {ORDER[order]}")


def test_headline_map_at_30_percent(headline_context):
    """dist2 from scipy alone; nearest by its distance everywhere and by the tie rule on a sample of cells"""
    import torch

    ndimage = pytest.importorskip("scipy.ndimage")
    seg, size = headline_context, 364
    rng = np.random.default_rng(6320)
    occ = rng.random((size, size)) < 0.30
    edt = ndimage.distance_transform_edt(~occ)
    want_d2 = np.rint(edt * edt).astype(np.int64)
    cells = size * size
    dst = Dest(1, cells)
    seeds = seed_planes([occ], ROW, cells, rng)
    assert raw_clearance(seg, 1, dst, seeds=seeds.data_ptr(), seed_stride=cells) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    dist2, nearest = host["dist2"].view(np.int32).reshape(size, size), host["nearest"].view(np.int32).reshape(size, size)
    assert np.array_equal(dist2, want_d2)
    assert int(host["counts"][0]) == int(occ.sum())
    rr, cc = np.mgrid[0:size, 0:size]
    nr, nc = nearest // size, nearest % size
    assert nearest.min() >= 0 and occ[nr, nc].all()
    assert np.array_equal((rr - nr) ** 2 + (cc - nc) ** 2, want_d2)
    want_m = np.sqrt(want_d2.astype(np.float32)) * np.float32(seg.resolution)
    assert np.array_equal(host["distance"], want_m.view(np.uint32).reshape(-1))
    occupied = np.argwhere(occ)  # (ascending (row, col): the first minimum is the tie rule)
    ties = 0
    for r, c in rng.integers(0, size, (200, 2)):
        d2 = (occupied[:, 0] - r) ** 2 + (occupied[:, 1] - c) ** 2
        k = int(np.argmin(d2))
        ties += int((d2 == d2[k]).sum() > 1)
        assert (int(nr[r, c]), int(nc[r, c])) == (int(occupied[k, 0]), int(occupied[k, 1])), (r, c)
    assert ties >= 10, ties  # (the sample holds cells with several equally near obstacles)


# ---------------------------------------------------------------- 4. right behind a batch, on the same stream, labels from its masks

def oracle_field(ref, cloud, labels, min_points, lo, hi, res):
    occ = expectation(ref, cloud, labels, min_points, lo, hi, 8, "row")[0] >= 0
    return occ, clearance_ref.expected_clearance(occ, 0, "row", np.float32(res))


def test_right_behind_a_batch_on_the_same_stream():
    import torch

    slots = [2, 0, 3]
    K = len(slots)
    length, res = GEOMETRY[79]
    clouds = [synth.hdl64_cloud(seed=6400 + k, n_az=90 + 10 * k) for k in range(K)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    seg = api.GroundSegmentation().init(length, res, n_slots=4, max_points=stride)
    pts = batch_points(clouds, stride)
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    plane_stride = seg.rows * seg.cols + 1
    dst = Dest(K, plane_stride)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(odom_z=0.0, on_torch_stream=True)
        out = seg.filter_batch(pts, n_pts, origins, base_z, slots=slots, want_masks=True)
        rc = raw_clearance(seg, K, dst, slots=slots, points=pts.data_ptr(), stride=stride, n_points=n_pts, masks=out.label_masks.data_ptr(), lo=0.2, hi=3.0)
        assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    occupied = 0
    for i in range(K):
        ref = oracle.OracleMap(length, res)
        lab = ref.filter_cloud(clouds[i], (0.0, 0.0, 0.0), -1.73)["label"]
        occ, want = oracle_field(ref, clouds[i], lab, 1, 0.2, 3.0, seg.resolution)
        occupied += int(occ.sum())
        check_map(host, i, want, ROW, seg.rows, seg.cols, plane_stride, f"behind the batch, cloud {i}")
    assert occupied >= 30, occupied
    seg.close()


# ---------------------------------------------------------------- 5. past the ring

def test_past_the_ring_back_to_back(cloud_scene, pattern_reference):
    """PARAM_RING + 1 calls on one stream without a synchronisation, every one with other inputs: clouds, slot lists, radii and orders of
    the cloud mode, and a seed-mode call in between"""
    import torch

    pats, free = pattern_reference
    sc, v = cloud_scene, cloud_scene["variant"](False)
    seg, stride = sc["seg"], sc["stride"]
    pts = points_tensor(v["given"], stride, _lib.GG_POINT16)
    lab = torch.from_numpy(sc["labels"]).cuda()
    cells = seg.rows * seg.cols
    n_all = len(CLOUD_PATTERNS)
    picks = [[0, 1, 2], [3, 4, 5], [5, 0], [1], [2, 3, 0, 4], [4, 1]][: PARAM_RING + 1]
    assert len(picks) == PARAM_RING + 1
    seeds = seed_planes([pats["w"], pats["comb"]], ROW, cells, np.random.default_rng(6500))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    calls = []
    with torch.cuda.stream(stream):
        for k, pick in enumerate(picks):
            order, max_cells = (ROW, COL)[k % 2], (0, 5, 12)[k % 3]
            sub_pts, sub_lab = pts[pick].contiguous(), lab[pick].contiguous()
            dst = Dest(len(pick), cells + 3)
            rc = raw_clearance(seg, len(pick), dst, slots=[CLOUD_SLOTS[i] for i in pick], points=sub_pts.data_ptr(), stride=stride,
                               n_points=[sc["n_pts"][i] for i in pick], labels=sub_lab.data_ptr(), min_points=2, lo=BAND[0], hi=BAND[1], max_cells=max_cells, order=order)
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
            calls.append((pick, order, max_cells, dst, sub_pts, sub_lab))
            if k == 2:
                seeded = Dest(2, cells)
                assert raw_clearance(seg, 2, seeded, seeds=seeds.data_ptr(), seed_stride=cells) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    for k, (pick, order, max_cells, dst, _, _) in enumerate(calls):
        host = dst.host()
        for j, i in enumerate(pick):
            check_map(host, j, derive(v["want"][i][1], 79, 79, max_cells, ORDER[order]), order, 79, 79, cells + 3, f"call {k}, cloud {CLOUD_PATTERNS[i]}")
    host = seeded.host()
    for j, name in enumerate(("w", "comb")):
        check_map(host, j, free[name], ROW, 79, 79, cells, f"the seed call, {name}")
    assert n_all == 6


# ---------------------------------------------------------------- 6. nothing else changes

def test_nothing_changes():
    import torch

    slots = [4, 1, 5, 2]
    K = len(slots)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000) for _ in range(2)]
    base = [synth.hdl64_cloud(seed=6600 + k, n_az=150 + 7 * k) for k in range(K)]
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
        if which == 0:  # the field between the two batches: on every map of the context (two of them fresh), of the batch, and of planes
            all_pts = torch.zeros((6, stride, 16), dtype=torch.uint8, device="cuda")  # (every point at the origin, z = 0: h = -0.1 on a fresh map)
            all_labels = torch.full((6, stride), 99, dtype=torch.uint8, device="cuda")
            every = seg.clearance_clouds(all_pts, [stride] * 6, labels=all_labels, slots=list(range(6)), min_height=-100.0, max_height=100.0)
            banded = seg.clearance_clouds(all_pts, [stride] * 6, labels=all_labels, slots=list(range(6)), min_height=-0.15, max_height=-0.05, nearest=False, distance=False)
            field = seg.clearance_clouds(pts[0], n_pts[0], masks=first.label_masks, slots=slots, min_points=2, min_height=0.3, max_height=2.5, max_cells=40)
            seg.clearance_planes(field.nearest, order="col", max_cells=3)
        # the lazily kept layers are still pending behind the calls: their first reader computes them, to the values of the twin
        assert lazy_count(seg) == K
        pending = seg.export_layers(lazy, slots=slots)
        assert lazy_count(seg) == 0
        second = seg.filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
        planes = seg.export_layers()
        torch.cuda.synchronize()
        if which == 0:  # one cell per map holds all the points; on the two fresh maps (0 and 3) the band admits exactly h = 0 - odom_z
            assert np.array_equal(every.n_occupied.cpu().numpy(), np.ones(6, np.int32))
            assert int(every.dist2.min().item()) == 0 and int(every.dist2.max().item()) < NONE
            got = banded.n_occupied.cpu().numpy()
            assert got[0] == got[3] == 1, got
            assert int(field.n_occupied.min().item()) > 0
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


# ---------------------------------------------------------------- 7. twice the same

def test_twice_the_same(cloud_scene, pattern_reference, seed_context):
    import torch

    pats, _ = pattern_reference
    sc, v = cloud_scene, cloud_scene["variant"](False)
    seg, stride, n = sc["seg"], sc["stride"], len(CLOUD_PATTERNS)
    pts = points_tensor(v["given"], stride, _lib.GG_POINT16)
    lab = torch.from_numpy(sc["labels"]).cuda()
    cells = 79 * 79
    seeds = seed_planes(list(pats.values()), COL, cells, np.random.default_rng(6700))
    runs = []
    for _ in range(2):
        a, b = Dest(n, cells + 3), Dest(len(pats), cells)
        assert raw_clearance(seg, n, a, slots=CLOUD_SLOTS, points=pts.data_ptr(), stride=stride, n_points=sc["n_pts"], labels=lab.data_ptr(), min_points=2,
                             lo=BAND[0], hi=BAND[1], max_cells=11) == 0
        assert raw_clearance(seed_context, len(pats), b, seeds=seeds.data_ptr(), seed_stride=cells, order=COL) == 0
        runs.append((a, b))
    torch.cuda.synchronize()
    for first, second in zip(runs[0], runs[1]):
        x, y = first.host(), second.host()
        for key in x:
            assert np.array_equal(x[key], y[key]), f"{key} differs between two runs"
        assert int(x["counts"].view(np.int32).max()) > 1000


# ---------------------------------------------------------------- 8. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=4096)
    seg.reset_maps(odom_z=0.4)
    clouds = [synth.hdl64_cloud(seed=6800 + k, n_az=40) for k in range(2)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    assert stride <= 4096
    warm_maps(seg, [4, 1], seed=6810, frames=1, n_az=40)
    before = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    labels = torch.full((2, stride), 99, dtype=torch.uint8, device="cuda")
    cells = seg.rows * seg.cols
    seeds = torch.zeros(7 * cells, dtype=torch.int32, device="cuda")
    dst = Dest(7, cells)
    P, Lb, S = pts.data_ptr(), labels.data_ptr(), seeds.data_ptr()

    def cloud(n=2, slots=None, first=0, fmt=_lib.GG_POINT16, points=P, stride=stride, n_points=n_pts, labels=Lb, masks=0, **kw):
        return raw_clearance(seg, n, dst, slots=slots, first_slot=first, fmt=fmt, points=points, stride=stride, n_points=n_points, labels=labels, masks=masks, **kw)

    def seed(n=2, seeds=S, seed_stride=cells, **kw):
        return raw_clearance(seg, n, dst, seeds=seeds, seed_stride=seed_stride, **kw)

    x = _lib.GGCloudClearance()
    x.n = 2
    assert seg._L.gg_clearance_clouds(None, C.byref(x), None) == INVALID
    assert seg._L.gg_clearance_clouds(seg._ctx, None, None) == INVALID
    assert cloud(n=-1) == INVALID and seed(n=-1) == INVALID
    # the ten shared members, through the shared frame
    assert cloud(slots=[1, 1]) == INVALID
    assert cloud(n_points=None) == INVALID
    assert cloud(fmt=2) == INVALID
    assert cloud(fmt=-1) == INVALID
    assert cloud(masks=Lb) == INVALID                 # both
    assert cloud(labels=0) == INVALID                 # neither
    assert cloud(labels=0, masks=Lb, stride=stride - 2, n_points=[10, 10]) == INVALID  # masks with a stride that is no multiple of 4
    assert cloud(n_points=[-1, 5]) == INVALID
    assert cloud(n_points=[5, stride + 1]) == INVALID
    assert cloud(n_points=[5, 4097]) == CAPACITY
    assert cloud(stride=4096, n_points=[5, 4097]) == CAPACITY
    assert cloud(stride=4097) == CAPACITY
    assert cloud(slots=[1, 6]) == CAPACITY
    assert cloud(slots=[-1, 2]) == CAPACITY
    assert cloud(first=5) == CAPACITY
    assert cloud(first=-1) == CAPACITY
    # the source of the occupancy
    assert cloud(points=0) == INVALID                 # neither source
    assert cloud(seeds=S, seed_stride=cells) == INVALID  # both
    assert seed(n_points=n_pts) == INVALID            # a cloud member in seed mode
    assert seed(labels=Lb) == INVALID
    assert seed(masks=Lb) == INVALID
    assert seed(transforms=np.zeros((2, 12))) == INVALID
    assert seed(slots=[0, 1]) == INVALID
    assert seed(seed_stride=cells - 1) == INVALID
    assert seed(n=7) == CAPACITY                      # more maps than the context has slots
    # the outputs and the options, in either mode
    for call in (cloud, seed):
        assert call(dist2=0) == INVALID
        assert call(plane_stride=cells - 1) == INVALID
        assert call(order=2) == INVALID
        assert call(order=-1) == INVALID
        assert call(max_cells=-1) == INVALID
    assert cloud(min_points=0) == INVALID
    assert cloud(min_points=-3) == INVALID
    assert cloud(lo=math.nan) == INVALID
    assert cloud(hi=math.nan) == INVALID
    assert cloud(n=0, points=0, n_points=None, labels=0, fmt=9, stride=10 ** 9, dist2=0, nearest=0, distance=0, counts=0, min_points=-1, order=7,
                 plane_stride=0, max_cells=-4, lo=math.nan) == 0  # n == 0: nothing to do, nothing to check
    assert seed(n=0, seeds=0, seed_stride=0, dist2=0, order=9) == 0
    torch.cuda.synchronize()
    assert dst.all_sentinel()
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    assert same_bits(before.cpu().numpy(), after.cpu().numpy())
    assert cloud(slots=[4, 1]) == 0, seg._L.gg_last_error(seg._ctx)  # ... and the same arguments without a mistake are accepted
    torch.cuda.synchronize()
    host = dst.host()
    assert 0 < int(host["counts"][0]) < cells and 0 < int(host["counts"][1]) < cells and np.all(host["counts"][2:] == SENTINEL)
    assert int(host["dist2"][: 2 * cells].view(np.int32).min()) == 0 and np.all(host["dist2"][2 * cells:] == SENTINEL)
    assert seed(n=6, max_cells=2 ** 31 - 1) == 0, seg._L.gg_last_error(seg._ctx)  # (every cell a seed)
    torch.cuda.synchronize()
    host = dst.host()
    assert np.all(host["dist2"][: 6 * cells] == 0) and np.all(host["counts"][:6] == cells) and np.all(host["dist2"][6 * cells:] == SENTINEL)
    assert np.array_equal(host["nearest"][:cells], np.arange(cells, dtype=np.uint32)) and np.all(host["distance"][: 6 * cells] == 0)
    assert fresh_count(seg) == fresh_before
    seg.close()


# ---------------------------------------------------------------- 9. the Python entry points

def test_python_entry_points(cloud_scene, pattern_reference):
    import torch

    sc, v = cloud_scene, cloud_scene["variant"](False)
    seg, stride, n = sc["seg"], sc["stride"], len(CLOUD_PATTERNS)
    pts = points_tensor(v["given"], stride, _lib.GG_POINT16)
    labels = torch.from_numpy(sc["labels"]).cuda()
    kw = dict(slots=CLOUD_SLOTS, min_points=2, min_height=BAND[0], max_height=BAND[1])
    a = seg.clearance_clouds(pts, sc["n_pts"], labels=labels, **kw)
    assert isinstance(a, api.ClearanceOutputs)
    for t, shape, dtype in ((a.dist2, (n, 79, 79), torch.int32), (a.nearest, (n, 79, 79), torch.int32), (a.distance, (n, 79, 79), torch.float32), (a.n_occupied, (n,), torch.int32)):
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda and t.is_contiguous()
    b = seg.clearance_clouds(pts, sc["n_pts"], labels=labels, order="col", max_cells=6, nearest=False, distance=False, on_torch_stream=False, **kw)
    assert b.nearest is None and b.distance is None
    again = seg.clearance_clouds(pts, sc["n_pts"], labels=labels, order="col", max_cells=6, nearest=False, distance=False, on_torch_stream=False, out=b, **kw)
    assert again is b
    clusters = seg.cluster_clouds(pts, sc["n_pts"], labels=labels, max_clusters=0, point_clusters=False, **kw)
    c = seg.clearance_planes(clusters.cell_cluster)
    with pytest.raises(ValueError):
        seg.clearance_clouds(pts, sc["n_pts"], labels=labels, order="fortran", **kw)
    with pytest.raises(ValueError):
        seg.clearance_clouds(pts, sc["n_pts"], labels=labels, max_cells=-1, **kw)
    with pytest.raises(ValueError):
        seg.clearance_clouds(pts, sc["n_pts"], **kw)
    with pytest.raises(ValueError):
        seg.clearance_clouds(pts, sc["n_pts"], labels=labels, nearest=False, out=a, **kw)  # (a plane that is not asked for)
    with pytest.raises(ValueError):
        seg.clearance_clouds(pts, sc["n_pts"], labels=labels, out=api.ClearanceOutputs(dist2=torch.empty((n, 79, 80), dtype=torch.int32, device="cuda")), **kw)
    with pytest.raises(ValueError):
        seg.clearance_planes(clusters.cell_cluster[:, :, :78].contiguous())
    with pytest.raises(ValueError):
        seg.clearance_planes(clusters.cell_cluster.float())
    with pytest.raises(ValueError):
        seg.clearance_planes(c.dist2, out=c)
    with pytest.raises(api.GroundGridError):
        seg.clearance_planes(torch.zeros((9, 79, 79), dtype=torch.int32, device="cuda"))  # (more planes than slots)
    torch.cuda.synchronize()
    seg.synchronize()
    for i, name in enumerate(CLOUD_PATTERNS):
        want = v["want"][i][1]
        assert np.array_equal(a.dist2[i].cpu().numpy(), want[0]) and np.array_equal(a.nearest[i].cpu().numpy(), want[1]), name
        assert np.array_equal(a.distance[i].cpu().numpy().view(np.uint32), want[2]) and int(a.n_occupied[i].item()) == want[3], name
        assert np.array_equal(b.dist2[i].cpu().numpy().T, derive(want, 79, 79, 6, "col")[0]), name
        for key in ("dist2", "nearest", "distance"):
            assert torch.equal(getattr(a, key)[i], getattr(c, key)[i]), (name, key)
    assert torch.equal(a.n_occupied, c.n_occupied)
    assert math.isinf(float(a.distance[CLOUD_PATTERNS.index("empty")].min().item()))
