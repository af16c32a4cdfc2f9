"""gg_match_planes (the best yaw candidate and translation of many scan planes over their field planes, in device memory) on the device.
Expected values come from numpy alone (tests/match_ref.py: one candidate at a time by one integer gather, the best by a lexicographic
sort; held against a count-plane correlation by tests/test_match_planes_cpu.py).  Every comparison is on bits: the six words of every row
of d_best, every word of every score volume, the words between a volume and its stride and behind the last row and volume."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402
from tests import fusion_ref, match_ref  # noqa: E402
from tests.test_export_layers_gpu import POSE, batch_points, fresh_count, same_bits, stride_of  # noqa: E402
from tests.test_fuse_states_gpu import GEOMETRY, MAX_POINTS, SIGNED_SENTINEL, pack, scan_cloud  # noqa: E402
from tests.test_split_clouds_gpu import PARAM_RING, lazy_count  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, GEOMETRY_ERR, CAPACITY = -1, -2, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
UNIT = match_ref.UNIT
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
FIELD_MAX = 32
SCENES = ("random", "empty", "full", "rim", "gone", "ties_a", "ties_b", "extremes", "pivot")
# the yaw candidates of a call, by their number: K = 1 is the NULL table; the third of three is no unit vector
TABLES = {1: None,
          3: np.concatenate([match_ref.IDENTITY, match_ref.rotation_table([np.radians(30.0)]), [[12000, -9000]]]).astype(np.int32),
          64: match_ref.rotation_table(np.concatenate([[0.0], np.linspace(-np.pi, np.pi, 63)]))}


# ---------------------------------------------------------------- scenes

@functools.lru_cache(maxsize=None)
def scene(name, side):
    """dict(scan, field: logical int32 [side, side]; shift, pivot) of one map"""
    rng = np.random.default_rng(2000 + 31 * side + SCENES.index(name))
    m = side // 2
    scan = np.where(rng.random((side, side)) < 0.05, rng.integers(1, 4, (side, side)), rng.integers(-2, 1, (side, side))).astype(np.int32)
    field = rng.integers(-20, 60, (side, side)).astype(np.int32)  # beyond both clamps of FIELD_MAX
    shift, pivot = (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (m, m)
    if name == "empty":  # no scan cell
        scan = np.minimum(scan, 0)
    elif name == "full":  # every cell a scan cell: the list is filled and flushed several times, every chunk seam is crossed
        scan[:] = 1
    elif name == "rim":  # scan cells on the rim: a rotation carries the corners outside and the shift brings some back
        scan[:] = -1
        scan[0, :] = scan[-1, :] = scan[:, 0] = scan[:, -1] = 1
        shift = (4, -3)
    elif name == "gone":  # scan cells within two cells of the pivot and a shift beyond the map: no window smaller than side / 2 - 4 reaches it
        scan[: m - 2] = scan[m + 3:] = scan[:, : m - 2] = scan[:, m + 3:] = 0
        scan[m, m] = 1
        shift = (side + 40, -3)
    elif name in ("ties_a", "ties_b"):  # one scan cell on the pivot (every rotation keeps it) under a symmetric field
        scan[:] = 0
        scan[m, m] = 2
        field[:] = -5
        for dy, dx in ((0, -1), (0, 1)) + (((-1, 0), (1, 0)) if name == "ties_a" else ()):
            field[m + dy, m + dx] = 9
        shift = (0, 0)
    elif name == "extremes":  # field words at both ends of the int32 range and next to both clamps
        field = rng.choice(np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, FIELD_MAX - 1, FIELD_MAX, FIELD_MAX + 1, I32_MAX - 1, I32_MAX], np.int64), (side, side)).astype(np.int32)
    elif name == "pivot":  # an off-centre pivot, in a corner region
        pivot = (2, side - 3)
    return dict(scan=scan, field=field, shift=shift, pivot=pivot)


@functools.lru_cache(maxsize=None)
def wanted(name, side, W, K, with_shift=True, with_pivot=True):
    s = scene(name, side)
    return match_ref.expected_match(s["scan"], s["field"], shift=s["shift"] if with_shift else None, pivot=s["pivot"] if with_pivot else None,
                                    rotations=TABLES[K], window=W, field_max=FIELD_MAX)


# ---------------------------------------------------------------- helpers

@pytest.fixture(scope="module")
def contexts():
    """one context per (side, slots), made on demand and shared: no call of this file but the drive's changes a map"""
    made = {}

    def get(side, n_slots=len(SCENES)):
        if (side, n_slots) not in made:
            length, res = GEOMETRY[side]
            seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=MAX_POINTS)
            assert seg.rows == seg.cols == side
            made[(side, n_slots)] = seg
        return made[(side, n_slots)]

    yield get
    for seg in made.values():
        seg.close()


class Dest:
    """sentinel-filled destinations of one call: n rows of six words and n volumes score_stride words apart, each with a few words behind"""

    def __init__(self, n, score_stride, slack=7):
        import torch

        self.n, self.score_stride = n, score_stride
        self.best = torch.full((6 * max(n, 1) + 5,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.scores = torch.full((max(n * score_stride + slack, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

    def host(self):
        return dict(best=self.best.cpu().numpy(), scores=self.scores.cpu().numpy())

    def all_sentinel(self):
        return bool((self.best == SIGNED_SENTINEL).all().item()) and bool((self.scores == SIGNED_SENTINEL).all().item())


def raw_match(seg, n, dest, scan, scan_stride, field, field_stride, window, order=ROW, shifts=None, pivots=None, rotations=None, field_max=FIELD_MAX,
              give_scores=True, stream=None, own=False, **over):
    """gg_match_planes as the C ABI has it (scan, field: device tensors or addresses, 0 / None = null; shifts, pivots: [n][2] or None;
    rotations: [K][2] or None); returns the status.  `over`: best, scores, score_stride, n_rotations in place of what follows from the rest"""
    import torch

    def address(t):
        return (t.data_ptr() if torch.is_tensor(t) else t) or None

    def host(a):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    x = _lib.GGPlaneMatches()
    x.n, x.d_scan, x.scan_stride, x.d_field, x.field_stride = n, address(scan), scan_stride, address(field), field_stride
    x.field_max, x.window, x.order = field_max, window, order
    keep = []
    for name, given in (("shifts", shifts), ("pivots", pivots), ("rotations", rotations)):
        if given is not None:
            a, p = host(given)
            keep.append(a)
            setattr(x, name, p)
    x.n_rotations = over.get("n_rotations", 0 if rotations is None else len(np.asarray(rotations).reshape(-1, 2)))
    x.d_best = address(over.get("best", dest.best))
    x.d_scores = address(over.get("scores", dest.scores if give_scores else 0))
    x.score_stride = over.get("score_stride", dest.score_stride)
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_match_planes(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check_map(host, i, want, dest, tag, give_scores=True):
    """row i and volume i of a downloaded Dest against match_ref.expected_match, and the words between the volume and the stride"""
    got = host["best"][6 * i: 6 * i + 6]
    assert got.tolist() == want["best"].tolist(), f"{tag}: map {i}: best {got.tolist()} != {want['best'].tolist()}"
    words = host["scores"][i * dest.score_stride: (i + 1) * dest.score_stride]
    if not give_scores:
        assert np.all(words == SIGNED_SENTINEL), f"{tag}: map {i}: the scores were not handed over and were written"
        return
    volume = want["scores"].ravel()
    bad = np.flatnonzero(words[: volume.size] != volume)
    assert len(bad) == 0, f"{tag}: map {i}: {len(bad)} scores differ, first at {np.unravel_index(bad[0], want['scores'].shape)}: {words[bad[0]]} != {volume[bad[0]]}"
    assert np.all(words[volume.size:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words behind the volume were written"


def check_tail(host, dest, tag):
    assert np.all(host["best"][6 * dest.n:] == SIGNED_SENTINEL), f"{tag}: the words behind the last row of d_best were written"
    assert np.all(host["scores"][dest.n * dest.score_stride:] == SIGNED_SENTINEL), f"{tag}: the words behind the last volume were written"


def scene_buffers(names, side, order, scan_stride, field_stride):
    got = [scene(name, side) for name in names]
    return (pack([g["scan"] for g in got], ORDER[order], scan_stride, slack=3), pack([g["field"] for g in got], ORDER[order], field_stride, slack=3),
            [g["shift"] for g in got], [g["pivot"] for g in got])


# ---------------------------------------------------------------- 1. every scene, on bits

CASES = [(side, W, K) for side in (20, 67, 128) for W in (0, 1, 10) for K in (1, 3)] + [(20, 32, 1), (20, 32, 3), (20, 1, 64)]


@pytest.mark.parametrize("order", [ROW, COL], ids=["row", "col"])
@pytest.mark.parametrize("side,W,K", CASES)
def test_every_scene_on_bits(contexts, side, W, K, order):
    """all scenes as the maps of one call, every buffer with a stride of its own.  20 x 20 is less than one chunk of the scan walk,
    67 x 67 ends on a ragged chunk, 128 x 128 cells fill the list eight times over"""
    import torch

    seg = contexts(side)
    cells, n = side * side, len(SCENES)
    assert cells < _lib.GG_MATCH_CHUNK or cells % _lib.GG_MATCH_CHUNK or cells > 4 * _lib.GG_MATCH_LIST
    volume = K * (2 * W + 1) ** 2
    scan_stride, field_stride, score_stride = cells + 3, cells + 8, volume + 5
    d_scan, d_field, shifts, pivots = scene_buffers(SCENES, side, order, scan_stride, field_stride)
    dst = Dest(n, score_stride)
    assert raw_match(seg, n, dst, d_scan, scan_stride, d_field, field_stride, W, order, shifts, pivots, TABLES[K]) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    for i, name in enumerate(SCENES):
        check_map(host, i, wanted(name, side, W, K), dst, f"{name} {side} W={W} K={K} {ORDER[order]}")
    check_tail(host, dst, "scenes")
    # what the scenes are there for
    D2 = (2 * W + 1) ** 2
    assert wanted("empty", side, W, K)["best"].tolist() == [0, 0, 0, 0, 0, K * D2]
    if W < side // 2 - 4:  # (a rotated cell lies within 2 * 2 cells of the pivot: the pairs here are no longer than sqrt(2))
        assert wanted("gone", side, W, K)["best"][[0, 1, 2, 3, 5]].tolist() == [0, 0, 0, 0, K * D2] and wanted("gone", side, W, K)["best"][4] > 0
    assert wanted("full", side, W, K)["best"][4] == cells
    if W >= 1:
        assert wanted("ties_a", side, W, K)["best"].tolist() == [0, -1, 0, 9, 1, 4 * K]
        assert wanted("ties_b", side, W, K)["best"].tolist() == [0, 0, -1, 9, 1, 2 * K]


# ---------------------------------------------------------------- 2. each nullable argument in turn, one map

@pytest.mark.parametrize("order", [ROW, COL], ids=["row", "col"])
def test_each_nullable_argument_in_turn(contexts, order):
    import torch

    side, W, K = 20, 3, 3
    seg = contexts(side)
    cells, names = side * side, ("random", "pivot", "rim")
    volume = K * (2 * W + 1) ** 2
    d_scan, d_field, shifts, pivots = scene_buffers(names, side, order, cells, cells)
    for with_shift, with_pivot, with_table, give in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                                                     (False, False, False, False)):
        k = K if with_table else 1
        dst = Dest(len(names), volume + 2)  # (the volume of one candidate lies in a stride made for three)
        assert raw_match(seg, len(names), dst, d_scan, cells, d_field, cells, W, order, shifts if with_shift else None, pivots if with_pivot else None,
                         TABLES[k], give_scores=give) == 0, seg._L.gg_last_error(seg._ctx)
        torch.cuda.synchronize()
        host = dst.host()
        for i, name in enumerate(names):
            check_map(host, i, wanted(name, side, W, k, with_shift, with_pivot), dst, f"shift {with_shift} pivot {with_pivot} table {with_table}: {name}", give)
        check_tail(host, dst, "nullable")
    # one map, one explicit candidate that is not the identity
    quarter = np.array([[0, UNIT]], np.int32)
    one = Dest(1, (2 * W + 1) ** 2)
    assert raw_match(seg, 1, one, d_scan, cells, d_field, cells, W, order, shifts[:1], pivots[:1], quarter) == 0
    torch.cuda.synchronize()
    s = scene("random", side)
    want = match_ref.expected_match(s["scan"], s["field"], shift=s["shift"], pivot=s["pivot"], rotations=quarter, window=W, field_max=FIELD_MAX)
    check_map(one.host(), 0, want, one, "n = 1")
    check_tail(one.host(), one, "n = 1")


# ---------------------------------------------------------------- 3. the ring, determinism, streams

def test_more_calls_than_the_ring_has_entries(contexts):
    """PARAM_RING + 3 calls back to back, each with shifts, pivots and a table of its own: an entry is reused only when its call has passed"""
    import torch

    side, W = 67, 2
    seg = contexts(side)
    cells, names = side * side, ("random", "rim", "pivot")
    d_scan, d_field, _, _ = scene_buffers(names, side, ROW, cells, cells)
    calls = []
    for j in range(PARAM_RING + 3):
        shifts = [(j - 3, 2 - j)] * 3
        pivots = [(5 + 7 * j, 60 - 6 * j)] * 3
        table = match_ref.rotation_table([0.0, np.radians(3.0 * (j + 1))])
        calls.append((shifts, pivots, table, Dest(3, 2 * (2 * W + 1) ** 2)))
    torch.cuda.synchronize()
    for shifts, pivots, table, dst in calls:
        assert raw_match(seg, 3, dst, d_scan, cells, d_field, cells, W, ROW, shifts, pivots, table) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    for j, (shifts, pivots, table, dst) in enumerate(calls):
        host = dst.host()
        for i, name in enumerate(names):
            s = scene(name, side)
            want = match_ref.expected_match(s["scan"], s["field"], shift=shifts[i], pivot=pivots[i], rotations=table, window=W, field_max=FIELD_MAX)
            check_map(host, i, want, dst, f"call {j}: {name}")
        check_tail(host, dst, f"call {j}")


def test_two_runs_byte_for_byte(contexts):
    import torch

    side, W, K = 128, 10, 3
    seg = contexts(side)
    cells, n = side * side, len(SCENES)
    d_scan, d_field, shifts, pivots = scene_buffers(SCENES, side, COL, cells, cells)
    runs = [Dest(n, K * (2 * W + 1) ** 2) for _ in range(2)]
    for dst in runs:
        assert raw_match(seg, n, dst, d_scan, cells, d_field, cells, W, COL, shifts, pivots, TABLES[K]) == 0
    torch.cuda.synchronize()
    a, b = runs[0].host(), runs[1].host()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{key} differs between two runs"
    assert a["best"][3] > 0


def test_on_a_caller_stream_and_on_the_contexts_own(contexts):
    import torch

    side, W, K = 20, 4, 3
    seg = contexts(side)
    cells, names = side * side, ("random", "full")
    d_scan, d_field, shifts, pivots = scene_buffers(names, side, ROW, cells, cells)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    mine, own = Dest(2, K * (2 * W + 1) ** 2), Dest(2, K * (2 * W + 1) ** 2)
    assert raw_match(seg, 2, mine, d_scan, cells, d_field, cells, W, ROW, shifts, pivots, TABLES[K], stream=stream.cuda_stream) == 0
    stream.synchronize()
    assert raw_match(seg, 2, own, d_scan, cells, d_field, cells, W, ROW, shifts, pivots, TABLES[K], own=True) == 0
    seg.synchronize()
    for dst, tag in ((mine, "caller stream"), (own, "own stream")):
        host = dst.host()
        for i, name in enumerate(names):
            check_map(host, i, wanted(name, side, W, K), dst, f"{tag}: {name}")
        check_tail(host, dst, tag)


# ---------------------------------------------------------------- 4. nothing else changes

def test_nothing_changes():
    """twin contexts run the same filter calls; one of them matches planes in between.  Layers, pending layers, labels, counts, scores and
    positions of the two are the same bits"""
    import torch

    side, K = 67, 3
    length, res = GEOMETRY[side]
    segs = [api.GroundSegmentation().init(length, res, n_slots=K, max_points=MAX_POINTS) for _ in range(2)]
    clouds = [[scan_cloud(9300 + k, (0.0, 0.0)) for k in range(K)], [scan_cloud(9310 + k, (0.6, -0.4)) for k in range(K)]]
    pts = [batch_points(c, MAX_POINTS) for c in clouds]
    n_pts = [[len(c) for c in batch] for batch in clouds]
    origins, base_z = np.zeros((2, 3), np.float32), np.full(2, -1.73)
    lazy = ["maxGroundHeight", "groundCandidates", "planeDist"]
    names = ("random", "rim", "pivot")
    d_scan, d_field, shifts, pivots = scene_buffers(names, side, ROW, side * side, side * side)
    d_scan, d_field = d_scan[: K * side * side].view(K, side, side), d_field[: K * side * side].view(K, side, side)
    results = []
    for which, seg in enumerate(segs):
        seg.reset_maps(odom_z=0.1)
        seg.set_scoring(slots=[0, 1])
        seg.move_maps([(0.7, -0.4), (0.0, 0.4)], [POSE] * 2)
        seg.filter_batch(pts[0][:2].contiguous(), n_pts[0][:2], origins, base_z, slots=[0, 1], want_masks=True)  # (map 2 stays fresh)
        assert lazy_count(seg) == 2 and fresh_count(seg) == 1
        if which == 0:  # the calls between the two batches, on as many planes as the context has maps
            first = seg.match_planes(d_scan, d_field, shifts=shifts, pivots=pivots, rotations=TABLES[3], window=1, field_max=FIELD_MAX, scores=True, on_torch_stream=True)
            seg.match_planes(d_scan.transpose(1, 2).contiguous(), d_field.transpose(1, 2).contiguous(), order="col", window=5, on_torch_stream=True)
            assert lazy_count(seg) == 2 and fresh_count(seg) == 1
        pending = seg.export_layers(lazy, slots=[0, 1])
        assert lazy_count(seg) == 0
        after = seg.filter_batch(pts[1][:2].contiguous(), n_pts[1][:2], origins, base_z, slots=[0, 1])
        layers = seg.export_layers()
        torch.cuda.synchronize()
        if which == 0:
            assert first.best.tolist() == [wanted(name, side, 1, 3)["best"].tolist() for name in names]
        results.append(dict(fresh=fresh_count(seg), pending=pending.cpu().numpy(), planes=layers.cpu().numpy(), labels=after.labels.cpu().numpy(),
                            counts=after.counts.cpu().numpy(), scores=seg.scores_raw(), positions=[seg.map(s).getPosition() for s in range(K)]))
    a, b = results
    assert a["fresh"] == b["fresh"] == 1
    assert same_bits(a["pending"], b["pending"]) and same_bits(a["planes"], b["planes"]) and a["planes"].shape[1] == 11
    assert np.array_equal(a["counts"], b["counts"]) and a["positions"] == b["positions"]
    for k in range(2):
        assert np.array_equal(a["labels"][k, : n_pts[1][k]], b["labels"][k, : n_pts[1][k]])
    assert np.array_equal(a["scores"][0], b["scores"][0]) and np.array_equal(a["scores"][1], b["scores"][1]) and a["scores"][0].sum() == 4
    for seg in segs:
        seg.close()


# ---------------------------------------------------------------- 5. errors change nothing

def test_errors_change_nothing(contexts):
    import torch

    side, W, K = 20, 2, 3
    seg = contexts(side, n_slots=5)
    cells, n = side * side, 3
    stride, volume = cells + 8, K * (2 * W + 1) ** 2
    d_scan, d_field, shifts, pivots = scene_buffers(("random", "rim", "pivot"), side, ROW, stride, stride)
    before = [t.clone() for t in (d_scan, d_field)]
    dst = Dest(n, volume + 4)
    fresh_before, lazy_before = fresh_count(seg), lazy_count(seg)

    def call(n=n, scan=d_scan, scan_stride=stride, field=d_field, field_stride=stride, window=W, order=ROW, shifts=shifts, pivots=pivots, rotations=TABLES[K], **kw):
        return raw_match(seg, n, dst, scan, scan_stride, field, field_stride, window, order, shifts, pivots, rotations, **kw)

    x = _lib.GGPlaneMatches()
    x.n = n
    assert seg._L.gg_match_planes(None, C.byref(x), None) == INVALID
    assert seg._L.gg_match_planes(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(scan=0) == INVALID
    assert call(field=0) == INVALID
    assert call(best=0) == INVALID
    assert call(scan_stride=cells - 1) == INVALID
    assert call(field_stride=cells - 1) == INVALID
    assert call(score_stride=volume - 1) == INVALID
    assert call(order=2) == INVALID
    assert call(order=-1) == INVALID
    assert call(window=-1) == INVALID
    assert call(window=33) == INVALID
    assert call(field_max=0) == INVALID
    assert call(field_max=-7) == INVALID
    top = (2 ** 31 - 1) // cells  # the overflow limit at its edge
    assert call(field_max=top + 1) == INVALID
    assert call(field_max=2 ** 31 - 1) == INVALID
    for bad in ((-1, 3), (side, 3), (3, -1), (3, side)):
        assert call(pivots=[pivots[0], bad, pivots[2]]) == INVALID, bad
    assert call(n_rotations=0) == INVALID  # (a table without candidates)
    assert call(n_rotations=-2) == INVALID
    assert call(n_rotations=65) == INVALID
    assert call(rotations=None, n_rotations=1) == INVALID  # (candidates without a table)
    for bad in ((UNIT + 1, 0), (0, -UNIT - 1), (I32_MIN, 0), (0, I32_MAX)):
        assert call(rotations=[(UNIT, 0), bad, (0, UNIT)]) == INVALID, bad
    assert call(n=6, shifts=[(0, 0)] * 6, pivots=[(1, 1)] * 6) == CAPACITY  # (more maps than the context has)
    # each pair of buffers that may not overlap: an output with an input, the outputs with each other
    for name in ("best", "scores"):
        for inp in (d_scan, d_field):
            assert call(**{name: inp}) == INVALID, name
            assert call(**{name: inp.data_ptr() + 4 * ((n - 1) * stride + cells - 1)}) == INVALID, name  # (the last cell of the last plane)
    assert call(best=dst.scores) == INVALID
    assert call(best=dst.scores.data_ptr() + 4 * ((n - 1) * (volume + 4) + volume - 1)) == INVALID  # (the last word of the last volume)
    assert call(scores=dst.best) == INVALID
    assert call(scores=dst.best.data_ptr() + 4 * (6 * n - 1)) == INVALID  # (the last word of the last row)
    assert call(n=0, scan=0, field=0, best=0, scan_stride=0, order=9, window=-4, field_max=0, n_rotations=99) == 0  # n == 0: nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel() and all(torch.equal(t, b) for t, b in zip((d_scan, d_field), before))
    assert fresh_count(seg) == fresh_before and lazy_count(seg) == lazy_before
    # ... and the same arguments without a mistake are accepted, at the edge of the limit and of the ranges too; the inputs may be one
    # buffer; the words behind an output belong to the caller; without d_scores its stride is not looked at
    assert call() == 0, seg._L.gg_last_error(seg._ctx)
    assert call(field_max=top) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(field=d_scan) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(window=32, give_scores=False, score_stride=0) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(rotations=[(UNIT, UNIT), (-UNIT, -UNIT)], pivots=[(0, 0), (side - 1, side - 1), (0, side - 1)]) == 0, seg._L.gg_last_error(seg._ctx)
    both = torch.full((6 * n + n * volume + 2,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")  # the rows, and right behind them the volumes
    assert call(best=both, scores=both.data_ptr() + 4 * 6 * n, score_stride=volume) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert not dst.all_sentinel()
    got = both.cpu().numpy()
    assert np.all(got[: 6 * n + n * volume] != SIGNED_SENTINEL) and np.all(got[6 * n + n * volume:] == SIGNED_SENTINEL)


def test_the_limit_at_its_edge_is_computed_right(contexts):
    """field_max at the largest accepted value, every field word above it, every cell a scan cell: S* = field_max * rows * cols fits"""
    import torch

    side = 20
    seg = contexts(side)
    cells = side * side
    top = (2 ** 31 - 1) // cells
    scan, field = np.ones((side, side), np.int32), np.full((side, side), I32_MAX, np.int32)
    dst = Dest(1, 9)
    assert raw_match(seg, 1, dst, pack([scan], "row", cells), cells, pack([field], "row", cells), cells, 1, ROW, field_max=top) == 0
    torch.cuda.synchronize()
    want = match_ref.expected_match(scan, field, window=1, field_max=top)
    assert want["best"].tolist() == [0, 0, 0, top * cells, cells, 1] and top * cells > 2 ** 31 - 1 - cells
    check_map(dst.host(), 0, want, dst, "the limit")


# ---------------------------------------------------------------- 6. the chain on real data

def test_the_chain_from_a_drive(contexts):
    """three frames on two maps: move, filter, trace, then match_planes(state, previous evidence, the shift of move_maps put off by (2, -1))
    and fuse_states with the corrected shift, every call on one stream; d_best and the fused planes are held to the two references"""
    import torch

    side, K, W = 128, 2, 4
    seg = contexts(side, n_slots=K)
    seg.reset_maps(odom_z=0.0)
    p = fusion_ref.params(hit=4, miss=3, free_threshold=-2, occ_threshold=4)
    fuse = {k: p[k] for k in ("hit", "miss", "decay", "free_threshold", "occ_threshold")}
    track = np.array([[(0.0, 0.0), (0.0, 0.0)], [(1.1, -0.8), (-0.5, 0.4)], [(2.5, -0.9), (-1.9, 1.5)]])
    table = api.rotation_table(np.radians([0.0, -1.0, 1.0]))
    evidence, outs, log = None, [api.FusionOutputs(), api.FusionOutputs()], []
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for f in range(len(track)):
            true_shifts = seg.move_maps(track[f], [POSE] * K, on_torch_stream=True)
            clouds = [scan_cloud(9700 + 10 * f + k, track[f, k]) for k in range(K)]
            stride = stride_of(clouds)
            pts, n_pts = batch_points(clouds, stride), [len(c) for c in clouds]
            origins = np.concatenate([track[f], np.full((K, 1), 1.7)], axis=1).astype(np.float32)
            out = seg.filter_batch(pts, n_pts, origins, np.full(K, -1.73), want_masks=True)
            vis = seg.visibility_clouds(pts, n_pts, origins, masks=out.label_masks, min_height=0.2, max_height=3.0)
            entry = dict(state=vis.state.clone(), true=np.array(true_shifts))
            shifts = np.array(true_shifts)
            if evidence is not None:
                wrong = shifts + np.array([2, -1])
                match = seg.match_planes(vis.state, evidence, shifts=wrong, rotations=table, window=W, field_max=p["e_max"], scores=True, on_torch_stream=True)
                best = match.best.cpu().numpy()  # (the corrected shift is a host argument of the next call)
                shifts = wrong + best[:, 1:3]
                entry.update(wrong=wrong, best=best, scores=match.scores.cpu().numpy(), prior=evidence.clone())
            fused = seg.fuse_states(vis.state, evidence, shifts=shifts, out=outs[f % 2], on_torch_stream=True, **fuse)
            evidence = fused.evidence
            entry.update(used=shifts, evidence=evidence.clone(), fused=fused.state.clone())
            log.append(entry)
    torch.cuda.synchronize()
    matched = scored = 0
    for f, e in enumerate(log):
        state = e["state"].cpu().numpy()
        for k in range(K):
            if "best" in e:
                want = match_ref.expected_match(state[k], e["prior"][k].cpu().numpy(), shift=e["wrong"][k], rotations=table, window=W, field_max=p["e_max"])
                assert e["best"][k].tolist() == want["best"].tolist(), f"frame {f}, map {k}"
                assert np.array_equal(e["scores"][k], want["scores"]), f"frame {f}, map {k}"
                assert want["best"][4] > 10  # a scan with cells to lay over the grid
                matched += 1
                scored += int(want["best"][3])
            prior = log[f - 1]["evidence"][k].cpu().numpy() if f else None
            fusion = fusion_ref.expected_fusion(state[k], prior, e["used"][k], p)
            assert np.array_equal(e["evidence"][k].cpu().numpy(), fusion["evidence"]) and np.array_equal(e["fused"][k].cpu().numpy(), fusion["fused"]), f"frame {f}, map {k}"
    assert matched == 4 and scored > 0


# ---------------------------------------------------------------- 7. the Python entry point

def test_python_entry_point(contexts):
    import torch

    side, names, W = 20, ("random", "rim", "pivot", "ties_a"), 3
    n = len(names)
    seg = contexts(side)
    d_scan, d_field, shifts, pivots = scene_buffers(names, side, ROW, side * side, side * side)
    d_scan, d_field = d_scan[: n * side * side].view(n, side, side), d_field[: n * side * side].view(n, side, side)
    angles = np.radians([0.0, 30.0, -90.0])
    table = api.rotation_table(angles)
    assert table.dtype == np.int32 and np.array_equal(table, match_ref.rotation_table(angles))
    a = seg.match_planes(d_scan, d_field, shifts=shifts, pivots=pivots, rotations=table, window=W, field_max=FIELD_MAX, scores=True, on_torch_stream=True)
    assert isinstance(a, api.MatchOutputs)
    for t, shape in ((a.best, (n, 6)), (a.scores, (n, 3, 2 * W + 1, 2 * W + 1))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    b = seg.match_planes(d_scan, d_field, on_torch_stream=True)
    assert b.scores is None and tuple(b.best.shape) == (n, 6)
    c = seg.match_planes(d_scan.transpose(1, 2).contiguous(), d_field.transpose(1, 2).contiguous(), shifts=np.array(shifts), pivots=pivots, rotations=table.tolist(),
                         window=W, field_max=FIELD_MAX, order="col", scores=True, on_torch_stream=True)
    again = seg.match_planes(d_scan, d_field, shifts=shifts, pivots=pivots, rotations=table, window=W, field_max=FIELD_MAX, scores=True, out=a)
    assert again is a
    seg.synchronize()
    torch.cuda.synchronize()
    for i, name in enumerate(names):
        s = scene(name, side)
        want = match_ref.expected_match(s["scan"], s["field"], shift=s["shift"], pivot=s["pivot"], rotations=table, window=W, field_max=FIELD_MAX)
        for got in (a, c):
            assert got.best[i].tolist() == want["best"].tolist(), name
            assert np.array_equal(got.scores[i].cpu().numpy(), want["scores"]), name
        plain = match_ref.expected_match(s["scan"], s["field"], **match_ref.DEFAULTS)
        assert b.best[i].tolist() == plain["best"].tolist(), name
    # bad arguments are refused before the call
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, out=api.MatchOutputs(best=d_scan), field=d_field)
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, d_field, out=a)  # (scores that are not asked for)
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, d_field, scores=True, out=api.MatchOutputs(scores=torch.empty((n, 1, 3, 3), dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError):
        seg.match_planes(d_scan.to(torch.int64), d_field)
    with pytest.raises(ValueError):
        seg.match_planes(d_scan[:, :, :19], d_field)
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, d_field[:2])
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, d_field, shifts=shifts[:2])
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, d_field, pivots=[(0, 0), (0, side), (1, 1), (2, 2)])
    with pytest.raises(ValueError):
        seg.match_planes(d_scan, d_field, rotations=[(UNIT + 1, 0)])
    with pytest.raises(api.GroundGridError):  # more planes than the context has maps: the library's GG_ERR_CAPACITY
        seg.match_planes(torch.cat([d_scan] * 3), torch.cat([d_field] * 3))
