"""gg_cluster_planes (the connected regions of any int32 plane of many maps, in device memory) on the device.  Expected values come from
numpy alone (tests/regions_ref.py, held together by tests/test_cluster_planes_cpu.py).  Every comparison is on bits: every cell of the id
and size planes, the four head words, every word of the records below min(K, max_regions); and the records from there on, the words
between rows * cols and a stride and the words behind the last plane keep their sentinel.

A non-square map cannot be made: gg_geometry has ONE length, so every map of this library is square.  The case that would run at 37 x 53
runs at 37 x 37 on content that is not symmetric under the transposition (a band of rows, a band of columns of another width, random
cells): a swap of rows and columns moves the bounds, the coordinate sums and the numbering of either order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402
from tests import clearance_ref, cluster_ref, regions_ref, tracks_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
SENTINEL = -77777
PARAM_RING = 4  # (gg_context.hip: entries of a call's parameter ring)
MAX, MIN = regions_ref.INT32_MAX, regions_ref.INT32_MIN
GG_ROUTE_NONE = 0x7FFFFFFF
GEOMETRY = {37: (12.0, 0.325), 79: (26.0, 0.33), 364: (120.0, 0.33)}  # side: (length, resolution)
N_SLOTS = {37: 6, 79: 14, 364: 2}


# ---------------------------------------------------------------- helpers

@pytest.fixture(scope="module")
def contexts():
    """one context per side, made on demand and shared: no call of this file changes a map"""
    made = {}

    def get(side):
        if side not in made:
            length, res = GEOMETRY[side]
            seg = api.GroundSegmentation().init(length, res, n_slots=N_SLOTS[side], max_points=1024)
            assert seg.rows == seg.cols == side
            made[side] = seg
        return made[side]

    yield get
    for seg in made.values():
        seg.close()


def lay(plane, order):
    return np.ascontiguousarray(plane if order == ROW else plane.T)


def pack(planes, order, stride, slack=0):
    """[rows, cols] planes as one device buffer: plane i where `order` puts it at i * stride, sentinels between and behind"""
    import torch

    host = np.full(max(len(planes) * stride + slack, 1), SENTINEL, np.int32)
    for i, a in enumerate(planes):
        host[i * stride: i * stride + a.size] = lay(np.asarray(a).astype(np.int32), order).ravel()
    return torch.from_numpy(host).cuda()


class Dest:
    """sentinel-filled destinations of one call"""

    FIELDS = ("plane", "size", "heads", "regions")

    def __init__(self, n, M, plane_stride, size_stride=None, slack=0):
        import torch

        def full(count):
            return torch.full((max(count, 1),), SENTINEL, dtype=torch.int32, device="cuda")

        self.n, self.M, self.plane_stride, self.size_stride = n, M, plane_stride, size_stride or plane_stride
        self.plane, self.size, self.heads = full(n * plane_stride + slack), full(n * self.size_stride + slack), full(4 * n + 3)
        self.regions = full(n * M * 12 + 12)  # (a fresh tensor is aligned far beyond 8 bytes)

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}

    def all_sentinel(self):
        return all(bool((getattr(self, k) == SENTINEL).all().item()) for k in self.FIELDS)


def raw_regions(seg, n, dest, seeds, seed_stride, lo=0, hi=MAX, conn=8, min_cells=1, order=ROW, values=None, value_stride=0, give_size=True,
                give_heads=True, give_regions=True, stream=None, **over):
    """gg_cluster_planes as the C ABI has it (device tensors or addresses, 0 / None = null); returns the status.  `over`: cell, plane_stride,
    size, size_stride, heads, regions, max_regions in place of `dest`'s"""
    import torch

    def address(t):
        return (t.data_ptr() if torch.is_tensor(t) else t) or None

    x = _lib.GGPlaneClusters()
    x.n, x.d_seeds, x.seed_stride = n, address(seeds), seed_stride
    x.lo, x.hi, x.connectivity, x.min_cells, x.order = lo, hi, conn, min_cells, order
    x.d_values, x.value_stride = address(values), value_stride
    x.d_cell_cluster, x.plane_stride = address(over.get("cell", dest.plane)), over.get("plane_stride", dest.plane_stride)
    x.d_cell_size, x.size_stride = address(over.get("size", dest.size if give_size else 0)), over.get("size_stride", dest.size_stride)
    x.d_heads = address(over.get("heads", dest.heads if give_heads else 0))
    x.d_regions = address(over.get("regions", dest.regions if give_regions and dest.M else 0))
    x.max_regions = over.get("max_regions", dest.M if give_regions else 0)
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_cluster_planes(seg._ctx, C.byref(x), C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check(host, want, dest, order, cells, tag, give_size=True, give_heads=True, give_regions=True):
    """a downloaded Dest against regions_ref's answers (one (plane, sizes, heads, records) per map), every word of it"""
    n, M = dest.n, dest.M
    for i, (plane, sizes, heads, rec) in enumerate(want):
        at = i * dest.plane_stride
        assert np.array_equal(host["plane"][at: at + cells], lay(plane, order).ravel()), f"{tag}: map {i}: the id plane"
        assert (host["plane"][at + cells: at + dest.plane_stride] == SENTINEL).all(), f"{tag}: map {i}: words between the planes"
        at = i * dest.size_stride
        if give_size:
            assert np.array_equal(host["size"][at: at + cells], lay(sizes, order).ravel()), f"{tag}: map {i}: the size plane"
            assert (host["size"][at + cells: at + dest.size_stride] == SENTINEL).all(), f"{tag}: map {i}: words between the size planes"
        if give_heads:
            assert host["heads"][4 * i: 4 * i + 4].tolist() == heads.tolist(), f"{tag}: map {i}: heads"
        if give_regions and M:
            got = host["regions"][i * M * 12: (i + 1) * M * 12].reshape(M, 12)
            k = min(len(rec), M)
            words = regions_ref.words_of(rec[:k])
            bad = np.nonzero((got[:k] != words).any(axis=1))[0]
            assert bad.size == 0, f"{tag}: map {i}: record {bad[0]}: {got[bad[0]].tolist()} != {words[bad[0]].tolist()}"
            assert (got[k:] == SENTINEL).all(), f"{tag}: map {i}: a record at or beyond min(K, max_regions) was written"
    assert (host["plane"][n * dest.plane_stride:] == SENTINEL).all() and (host["heads"][4 * n:] == SENTINEL).all(), tag
    assert (host["regions"][n * M * 12:] == SENTINEL).all(), tag
    if not give_size:
        assert (host["size"] == SENTINEL).all(), tag
    else:
        assert (host["size"][n * dest.size_stride:] == SENTINEL).all(), tag
    if not give_heads:
        assert (host["heads"] == SENTINEL).all(), tag
    if not give_regions:
        assert (host["regions"] == SENTINEL).all(), tag


def run_and_check(seg, seeds_planes, tag, lo=0, hi=MAX, conn=8, min_cells=1, order=ROW, values_planes=None, M=256, pad=0, give_size=True,
                  give_heads=True, give_regions=True, want=None):
    import torch

    n, cells = len(seeds_planes), seg.rows * seg.cols
    seeds = pack(seeds_planes, order, cells + pad, slack=pad)
    values = pack(values_planes, order, cells + 2 * pad, slack=pad) if values_planes is not None else None
    dest = Dest(n, M, cells + 3 * pad, cells + 4 * pad, slack=pad)
    rc = raw_regions(seg, n, dest, seeds, cells + pad, lo, hi, conn, min_cells, order, values, cells + 2 * pad, give_size, give_heads, give_regions)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    if want is None:
        want = [regions_ref.expected_regions(s, lo, hi, conn, min_cells, ORDER[order], None if values_planes is None else values_planes[i])
                for i, s in enumerate(seeds_planes)]
    check(dest.host(), want, dest, order, cells, tag, give_size, give_heads, give_regions)
    assert bool((seeds == pack(seeds_planes, order, cells + pad, slack=pad)).all().item()), f"{tag}: the seeds changed"
    return want, dest


# ---------------------------------------------------------------- 1. the patterns, fourteen maps in one call

@pytest.fixture(scope="module")
def pattern_labels():
    pats = cluster_ref.patterns(79, 79)
    assert len(pats) == 14
    labels = {}

    def get(conn, order):
        if (conn, order) not in labels:
            labels[conn, order] = [cluster_ref.label_plane(occ, conn, ORDER[order]) for occ in pats.values()]
        return labels[conn, order]

    return pats, get


@pytest.mark.parametrize("min_cells", [1, 2, 5])
@pytest.mark.parametrize("order", [ROW, COL])
@pytest.mark.parametrize("conn", [4, 8])
def test_patterns(contexts, pattern_labels, conn, order, min_cells):
    seg = contexts(79)
    pats, labels = pattern_labels
    rr, cc = np.mgrid[0:79, 0:79]
    values = [((rr * 31 + cc * 17 + 7 * i) % 23 - 11).astype(np.int32) for i in range(len(pats))]  # with ties inside every larger region
    seeds = [np.where(occ, i, -1 - i) for i, occ in enumerate(pats.values())]  # (members hold the map's number: lo = 0 selects them)
    want = [regions_ref.regions_of_labels(lab, min_cells, ORDER[order], values[i]) for i, lab in enumerate(labels(conn, order))]
    names = list(pats)
    board = want[names.index("checkerboard")]
    if conn == 4:  # 3121 components of one cell: all of them regions, or all of them dropped
        assert board[2].tolist() == ([3121, 0, 3121, 3121] if min_cells == 1 else [0, 3121, 3121, 0])
    run_and_check(seg, seeds, f"patterns conn {conn} {ORDER[order]} min_cells {min_cells}", conn=conn, min_cells=min_cells, order=order,
                  values_planes=values, M=256, pad=5, want=want)  # (check() holds the first record past max_regions to its sentinel)


def test_patterns_without_the_optional_outputs(contexts, pattern_labels):
    """min_cells == 1 and no d_cell_size: the size and filter launches do not run; no heads, no table"""
    seg = contexts(79)
    pats, labels = pattern_labels
    seeds = [np.where(occ, 0, -1) for occ in pats.values()]
    want = [regions_ref.regions_of_labels(lab, 1, "row") for lab in labels(8, ROW)]
    run_and_check(seg, seeds, "plane alone", give_size=False, give_heads=False, give_regions=False, want=want)
    run_and_check(seg, seeds, "plane and heads", give_size=False, give_regions=False, want=want)
    run_and_check(seg, seeds, "plane and table", give_size=False, give_heads=False, M=7, want=want)


# ---------------------------------------------------------------- 2. rows and columns, strides, ranges, values

def lopsided(seed, side=37):
    """{-1, 0, 1} on a plane that no transposition maps to itself: a band of three rows, a band of five columns, random cells"""
    rng = np.random.default_rng(seed)
    p = rng.choice(np.array([-1, 0, 1], dtype=np.int32), size=(side, side), p=[0.5, 0.2, 0.3])
    p[4:7, 2:30] = 1
    p[9:33, 20:25] = 0
    p[side - 1, :11] = 1
    return p


@pytest.mark.parametrize("order", [ROW, COL])
def test_rows_are_not_columns_and_strides(contexts, order):
    seg = contexts(37)
    seeds = [lopsided(7100 + i) for i in range(5)]
    for s in seeds:
        a = regions_ref.expected_regions(s, connectivity=4, min_cells=3)[3]
        assert not np.array_equal(a["sum_row"], a["sum_col"]) and not np.array_equal(a["row_min"], a["col_min"])
    values = [np.random.default_rng(7200 + i).integers(-9, 9, size=(37, 37)).astype(np.int32) for i in range(5)]
    run_and_check(seg, seeds, f"lopsided {ORDER[order]}", conn=4, min_cells=3, order=order, values_planes=values, M=40, pad=11)
    run_and_check(seg, seeds, f"lopsided {ORDER[order]} conn 8", conn=8, min_cells=2, order=order, values_planes=values, M=40, pad=64)


@pytest.mark.parametrize("lo,hi", [(0, MAX), (1, 1), (-1, -1), (-1, 0), (MIN, MAX)])
def test_three_valued_plane(contexts, lo, hi):
    seg = contexts(37)
    seeds = [lopsided(7300 + i) for i in range(3)]
    want, _ = run_and_check(seg, seeds, f"[{lo}, {hi}]", lo=lo, hi=hi, conn=8, min_cells=2, order=ROW, M=64, pad=3)
    members = [int(((s >= lo) & (s <= hi)).sum()) for s in seeds]
    assert [int(w[2][2]) for w in want] == members and all(m > 0 for m in members)
    if (lo, hi) == (MIN, MAX):
        assert all(w[2].tolist() == [1, 0, 37 * 37, 37 * 37] for w in want)


def test_value_planes(contexts):
    """ties, the ends of the int32 range, negative values, and GG_ROUTE_NONE on whole regions"""
    seg = contexts(37)
    seeds = [lopsided(7400 + i) for i in range(4)]
    rng = np.random.default_rng(7450)
    ties = rng.integers(0, 3, size=(37, 37)).astype(np.int32)
    ends = rng.choice(np.array([MIN, MIN + 1, -1, 0, 1, MAX - 1, MAX], dtype=np.int64), size=(37, 37)).astype(np.int32)
    negative = rng.integers(-2000000000, -1, size=(37, 37)).astype(np.int32)
    none = rng.integers(0, 500, size=(37, 37)).astype(np.int32)
    lab = cluster_ref.label_plane(seeds[3] >= 0, 8, "row")
    none[(lab >= 0) & (lab % 2 == 0)] = GG_ROUTE_NONE  # every other region holds GG_ROUTE_NONE alone
    values = [ties, ends, negative, none]
    for order in (ROW, COL):
        want, _ = run_and_check(seg, seeds, f"values {ORDER[order]}", conn=8, order=order, values_planes=values, M=128, pad=2)
        if order == ROW:
            rec = want[3][3]
            assert (rec["value_min"] == GG_ROUTE_NONE).sum() >= 2 and np.array_equal(rec["value_cell"][rec["value_min"] == GG_ROUTE_NONE],
                                                                                      rec["first_cell"][rec["value_min"] == GG_ROUTE_NONE])
            assert (want[1][3]["value_min"] == MIN).any() and (want[0][3]["value_min"] == 0).any()


# ---------------------------------------------------------------- 3. the full-size map: a thread of the scan owns more than one chunk

@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(7500)
    random = np.where(rng.random((364, 364)) < 0.6, 1, -1)
    spiral = np.where(cluster_ref.spiral(364, 364), 1, -1)
    values = rng.integers(-50, 50, size=(364, 364)).astype(np.int32)
    want = {conn: [regions_ref.expected_regions(s, 1, 1, conn, 4, "row", values) for s in (random, spiral)] for conn in (4, 8)}
    return [random, spiral], values, want


@pytest.mark.parametrize("conn", [4, 8])
def test_full_size_random_and_spiral(contexts, big, conn):
    seg = contexts(364)
    assert seg.rows * seg.cols > 65536
    seeds, values, want = big
    assert want[conn][1][2].tolist()[:2] == [1, 0] and want[conn][1][3]["cells"][0] > 60000  # the spiral: one region, the longest chains
    assert want[conn][0][2][0] > 256 or conn == 8
    run_and_check(seg, seeds, f"364 conn {conn}", lo=1, hi=1, conn=conn, min_cells=4, order=ROW, values_planes=[values, values], M=256, pad=1,
                  want=want[conn])


# ---------------------------------------------------------------- 4. agreement with gg_cluster_clouds, and the chain

def test_agreement_with_cluster_clouds():
    """gg_cluster_clouds on the scene of its own test, then gg_cluster_planes on its id plane with lo = 0: the same plane, and the same
    cells, bounds and first_cell"""
    import torch

    from tests import test_cluster_clouds_gpu as cc

    sc = cc.cluster_scene(_lib.GG_POINT16, False)
    seg, n = sc["seg"], len(sc["slots"])
    try:
        cells, M = seg.rows * seg.cols, 1024
        for order in (ROW, COL):
            dst = cc.Dest(n, cells, sc["stride"], M)
            rc = cc.raw_cluster(seg, n, sc["slots"], 0, sc["fmt"], sc["pts"].data_ptr(), sc["stride"], sc["n_pts"], dst, masks=sc["masks"].data_ptr(), conn=8,
                                order=order, min_points=cc.SCAN["min_points"], lo=cc.SCAN["lo"], hi=cc.SCAN["hi"])
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
            dest = Dest(n, M, cells)
            assert raw_regions(seg, n, dest, dst.planes, cells, conn=8, order=order, give_size=False) == 0, seg._L.gg_last_error(seg._ctx)
            torch.cuda.synchronize()
            assert torch.equal(dst.planes[: n * cells], dest.plane[: n * cells])
            table = dst.table.cpu().numpy().reshape(n, M, 8)
            counts, heads = dst.counts.cpu().numpy(), dest.heads.cpu().numpy()[: 4 * n].reshape(n, 4)
            got = dest.regions.cpu().numpy()[: n * M * 12].reshape(n, M, 12)
            assert np.array_equal(heads[:, 0], counts) and (heads[:, 1] == 0).all() and int(counts.max()) >= 20
            for i in range(n):
                k = min(int(counts[i]), M)
                assert np.array_equal(got[i, :k, :5], table[i, :k, [0, 2, 3, 4, 5]].T) and np.array_equal(got[i, :k, 5], table[i, :k, 7]), (order, i)
    finally:
        seg.close()


def test_chain_into_track_clusters_and_clearance_planes(contexts):
    import torch

    seg = contexts(37)
    seeds = [lopsided(7600 + i) for i in range(4)]
    for order in ("row", "col"):
        dev = torch.from_numpy(np.stack([lay(s, ROW if order == "row" else COL) for s in seeds]).astype(np.int32)).cuda()
        res = seg.cluster_planes(dev, lo=1, hi=1, min_cells=3, order=order, on_torch_stream=True)
        tracks = seg.track_clusters(res.cell_cluster, max_clusters=64, gate=1, cell_track=True, on_torch_stream=True, order=order)
        clear = seg.clearance_planes(res.cell_cluster, order=order, on_torch_stream=True)
        torch.cuda.synchronize()
        want = [regions_ref.expected_regions(s, 1, 1, 8, 3, order) for s in seeds]
        planes = np.stack([lay(w[0], ROW if order == "row" else COL) for w in want])
        assert np.array_equal(res.cell_cluster.cpu().numpy(), planes)
        recs, heads, cell_track = tracks_ref.track_maps(planes, M=64, g=1, order=order)
        assert np.array_equal(tracks.heads.cpu().numpy(), heads) and np.array_equal(tracks.cell_track.cpu().numpy(), cell_track)
        for i, r in enumerate(recs):
            assert np.array_equal(tracks.tracks[i, : len(r)].cpu().numpy(), np.ascontiguousarray(r).view(np.int32).reshape(len(r), 8)), (order, i)
            assert np.array_equal(r["cells"], want[i][3]["cells"][: len(r)]) and np.array_equal(r["sum_row"], want[i][3]["sum_row"][: len(r)])
        for i, w in enumerate(want):
            d2, near, dist, occupied = clearance_ref.expected_clearance(w[0] >= 0, 0, order, seg.resolution)
            assert np.array_equal(clear.dist2[i].cpu().numpy(), clearance_ref.as_plane(d2, order)), (order, i)
            assert np.array_equal(clear.nearest[i].cpu().numpy(), clearance_ref.as_plane(near, order)), (order, i)
            assert np.array_equal(clear.distance[i].cpu().numpy().view(np.uint32), clearance_ref.as_plane(dist, order)), (order, i)
            assert int(clear.n_occupied[i].item()) == occupied == int(w[2][3])


# ---------------------------------------------------------------- 5. determinism, the ring

def test_twice_the_same(contexts, big):
    import torch

    seg = contexts(364)
    seeds, values, _ = big
    cells = seg.rows * seg.cols
    s, v = pack(seeds, ROW, cells), pack([values, values], ROW, cells)
    runs = []
    for _ in range(2):
        dest = Dest(2, 256, cells)
        assert raw_regions(seg, 2, dest, s, cells, lo=1, hi=1, conn=8, min_cells=3, values=v, value_stride=cells) == 0
        torch.cuda.synchronize()
        runs.append(dest.host())
    assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in Dest.FIELDS)


def test_on_a_caller_stream_past_the_ring(contexts):
    import torch

    seg = contexts(37)
    cells, n = 37 * 37, 3
    stream = torch.cuda.Stream()
    rounds = []
    with torch.cuda.stream(stream):
        for k in range(PARAM_RING + 2):
            seeds = [lopsided(7700 + 10 * k + i) for i in range(n)]
            s, dest = pack(seeds, ROW, cells), Dest(n, 32, cells)
            assert raw_regions(seg, n, dest, s, cells, conn=4, min_cells=1 + k % 3, stream=stream.cuda_stream) == 0, seg._L.gg_last_error(seg._ctx)
            rounds.append((seeds, s, dest, 1 + k % 3))
    stream.synchronize()
    for k, (seeds, _, dest, m) in enumerate(rounds):
        check(dest.host(), [regions_ref.expected_regions(p, connectivity=4, min_cells=m) for p in seeds], dest, ROW, cells, f"round {k}")


@pytest.mark.parametrize("side", [37, 79, 364])
def test_tile_stage_gives_the_same_bits(contexts, pattern_labels, big, side):
    """both paths stay reachable (gg_debug_regions_tile): the plain merge and the tile-local stage in LDS in front of the
    flatten give the reference's answer, so the same bytes; 37, 79 and 364 are no multiples of the tile's 32"""
    seg = contexts(side)
    default = seg.debug_regions_tile()
    assert default in (0, 1)
    if side == 79:
        pats, labels = pattern_labels
        seeds = [np.where(occ, 0, -1) for occ in pats.values()]
        cases = [(dict(conn=conn, order=order, min_cells=2, M=256, pad=3), [regions_ref.regions_of_labels(lab, 2, ORDER[order]) for lab in labels(conn, order)])
                 for conn in (4, 8) for order in (ROW, COL)]
    elif side == 37:
        seeds = [lopsided(7650 + i) for i in range(6)]
        cases = [(dict(conn=conn, order=order, min_cells=1, M=64, pad=7, give_size=False), None) for conn in (4, 8) for order in (ROW, COL)]
    else:
        seeds, values, want = big
        cases = [(dict(lo=1, hi=1, conn=conn, min_cells=4, values_planes=[values, values], M=256, pad=1), want[conn]) for conn in (4, 8)]
    try:
        for kw, want in cases:
            hosts = []
            for tile in (0, 1):
                seg.debug_regions_tile(tile)
                want, dest = run_and_check(seg, seeds, f"side {side} tile {tile} {kw.get('conn')} {kw.get('order')}", want=want, **kw)
                hosts.append(dest.host())
            assert all(hosts[0][k].tobytes() == hosts[1][k].tobytes() for k in Dest.FIELDS)
    finally:
        seg.debug_regions_tile(default)


# ---------------------------------------------------------------- 6. refusals

def test_errors_change_nothing(contexts):
    import torch

    seg = contexts(37)
    cells, n, M = 37 * 37, 3, 8
    stride = cells + 4
    seeds_host = [lopsided(7800 + i) for i in range(n)]
    seeds, values = pack(seeds_host, ROW, stride), pack(seeds_host, ROW, stride)
    before = seeds.clone()
    dest = Dest(n, M, stride)
    base = dict(lo=0, hi=MAX, conn=8, min_cells=2, order=ROW, values=values, value_stride=stride)

    def call(n_=n, seeds_=seeds, seed_stride=stride, **kw):
        return raw_regions(seg, n_, dest, seeds_, seed_stride, **{**base, **kw})

    L = seg._L
    assert L.gg_cluster_planes(None, None, None) == INVALID and L.gg_cluster_planes(seg._ctx, None, None) == INVALID
    assert call(n_=-1) == INVALID
    assert call(seeds_=0) == INVALID and call(cell=0) == INVALID
    assert call(lo=1, hi=0) == INVALID and call(lo=MAX, hi=MIN) == INVALID
    for conn in (0, 6, 9, -8):
        assert call(conn=conn) == INVALID
    for order in (-1, 2):
        assert call(order=order) == INVALID
    assert call(seed_stride=cells - 1) == INVALID and call(plane_stride=cells - 1) == INVALID
    assert call(value_stride=cells - 1) == INVALID and call(size_stride=cells - 1) == INVALID and call(size_stride=0) == INVALID
    assert call(min_cells=0) == INVALID and call(min_cells=-3) == INVALID
    assert call(min_cells=2, give_size=False) == INVALID
    assert call(max_regions=-1) == INVALID and call(max_regions=0) == INVALID  # (d_regions is given)
    assert call(regions=dest.regions.data_ptr() + 4) == INVALID
    # overlap: an output on an input, an output on an output, by one word at the far end
    assert call(cell=seeds) == INVALID and call(size=seeds) == INVALID and call(cell=values) == INVALID
    assert call(size=dest.plane) == INVALID and call(heads=dest.plane) == INVALID and call(regions=dest.size) == INVALID
    assert call(cell=seeds.data_ptr() + 4 * ((n - 1) * stride + cells - 1)) == INVALID
    assert call(heads=dest.regions.data_ptr() + 4 * (n * M * 12 - 1)) == INVALID
    assert call(n_=N_SLOTS[37] + 1) == CAPACITY
    torch.cuda.synchronize()
    assert dest.all_sentinel() and torch.equal(seeds, before)
    assert b"gg_cluster_planes" in L.gg_last_error(seg._ctx)
    # n == 0 is fine before anything else is looked at; inputs may overlap each other; and the context still works
    assert raw_regions(seg, 0, dest, 0, 0, lo=1, hi=0, conn=5, min_cells=0, order=9, cell=0) == 0 and dest.all_sentinel()
    assert call(values=seeds) == 0
    torch.cuda.synchronize()
    check(dest.host(), [regions_ref.expected_regions(s, min_cells=2, values=s) for s in seeds_host], dest, ROW, cells, "after the refusals")


# ---------------------------------------------------------------- 7. Python

def test_python_entry_point(contexts):
    import torch

    seg = contexts(37)
    host = np.stack([lopsided(7900 + i) for i in range(3)]).astype(np.int32)
    seeds = torch.from_numpy(host).cuda()
    values = torch.from_numpy(np.random.default_rng(7950).integers(0, 40, size=host.shape).astype(np.int32)).cuda()
    res = seg.cluster_planes(seeds, min_cells=3, values=values, max_regions=16)
    seg.synchronize()
    want = [regions_ref.expected_regions(host[i], min_cells=3, values=values[i].cpu().numpy()) for i in range(3)]
    assert res.cell_cluster.shape == (3, 37, 37) and res.cell_size is not None and res.regions.shape == (3, 16, 12)
    for i, (plane, sizes, heads, rec) in enumerate(want):
        assert np.array_equal(res.cell_cluster[i].cpu().numpy(), plane) and np.array_equal(res.cell_size[i].cpu().numpy(), sizes)
        assert res.heads[i].cpu().numpy().tolist() == heads.tolist()
        table = res.table(i)
        assert table.dtype == api.REGION_DTYPE and table.tobytes() == rec[:16].tobytes()
        xy = res.centroids(i, seg.resolution, seg.length)
        k = np.arange(len(table))
        assert np.allclose(xy[:, 0], 0.5 * seg.length[0] - (rec["sum_row"][k] / rec["cells"][k] + 0.5) * seg.resolution)
        assert np.allclose(xy[:, 1], 0.5 * seg.length[1] - (rec["sum_col"][k] / rec["cells"][k] + 0.5) * seg.resolution)
    # out= reuses the tensors; the defaults leave the sizes out; state planes by range; column order
    again = seg.cluster_planes(seeds, min_cells=3, values=values, max_regions=16, out=res)
    assert again is res
    plain = seg.cluster_planes(seeds, lo=1, hi=1, max_regions=0)
    seg.synchronize()
    assert plain.cell_size is None and plain.regions is None
    assert np.array_equal(plain.cell_cluster[1].cpu().numpy(), regions_ref.expected_regions(host[1], 1, 1)[0])
    col = seg.cluster_planes(seeds.transpose(1, 2).contiguous(), lo=-1, hi=-1, connectivity=4, order="col", sizes=True, on_torch_stream=True)
    torch.cuda.synchronize()
    p, s, h, _ = regions_ref.expected_regions(host[2], -1, -1, 4, 1, "col")
    assert np.array_equal(col.cell_cluster[2].cpu().numpy(), p.T) and np.array_equal(col.cell_size[2].cpu().numpy(), s.T) and col.heads[2].tolist() == h.tolist()
    # refusals
    with pytest.raises(ValueError, match="seeds"):
        seg.cluster_planes(seeds, out=api.RegionOutputs(cell_cluster=seeds))
    with pytest.raises(ValueError, match="may not be outputs"):
        seg.cluster_planes(seeds, values=values, sizes=True, out=api.RegionOutputs(cell_size=values))
    with pytest.raises(ValueError, match="not asked for"):
        seg.cluster_planes(seeds, out=api.RegionOutputs(cell_size=torch.empty_like(seeds)))
    for bad in (dict(connectivity=6), dict(min_cells=0), dict(lo=2, hi=1), dict(order="xy"), dict(max_regions=-1), dict(lo=1.5), dict(values=values[:2])):
        with pytest.raises(ValueError):
            seg.cluster_planes(seeds, **bad)
    for bad in (seeds.cpu(), seeds.float(), seeds[:, :36], seeds[0]):
        with pytest.raises(ValueError):
            seg.cluster_planes(bad)
    with pytest.raises(_lib.GroundGridError):
        seg.cluster_planes(torch.cat([seeds, seeds, seeds]))  # 9 maps on 6 slots: GG_ERR_CAPACITY
