"""gg_footprint_planes (which headings of a vehicle footprint fit at every cell of many blocked planes, in device memory) on the device.
Expected values come from numpy alone (tests/footprint_ref.py: shifted copies of the padded blocked plane OR-ed together; held against
scipy's dilation and closed forms by tests/test_footprint_planes_cpu.py).  Every comparison is on bits: every word of every mask and fit
plane, the three counts of every map, the words between a plane and its stride and behind the last plane and the last counts."""
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
from tests import footprint_ref as ref, fusion_ref, route_ref  # noqa: E402
from tests.test_export_layers_gpu import POSE, batch_points, fresh_count, same_bits, stride_of  # noqa: E402
from tests.test_fuse_states_gpu import GEOMETRY, MAX_POINTS, SIGNED_SENTINEL, pack, scan_cloud  # noqa: E402
from tests.test_split_clouds_gpu import PARAM_RING, lazy_count  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
UNIT = ref.UNIT
SCENES = ref.SCENES
OUTPUTS = ("mask", "fit", "counts")
EMPTY_ROW = list(ref.EMPTY)


def table(rows):
    return np.array(rows, np.int32)


def small_spans():
    """2 x 1 cells ahead of the reference cell, 8 headings, R = 3: a footprint for the 20 x 20 maps"""
    return table(ref.rect_spans(ref.headings(8), ref.rect_of(2.0, 0.0, 0.5, 0.5, pad=0.3), 3))


def gap_spans():
    """the small footprint with headings 2 and 5 emptied: all-empty headings among non-empty ones"""
    t = small_spans()
    t[[2, 5]] = ref.EMPTY
    return t


# the span tables of the calls, by name
FOOTPRINTS = {
    "car": ref.car_spans(),                                                              # K = 32, R = 14
    "small": small_spans(),                                                              # K = 8, R = 3
    "gap": gap_spans(),
    "cell": table([[[0, 0]]]),                                                           # K = 1, R = 0: the cell itself
    "cell in 3": table([[EMPTY_ROW] * 3 + [[0, 0]] + [EMPTY_ROW] * 3]),                  # the same cell in a table of R = 3
    "radius 0": table([[[0, 0]], [EMPTY_ROW], [[0, 0]]]),                                # K = 3, R = 0, one heading empty
    "square": table([[[-32, 32]] * 65] * 2),                                             # K = 2, R = 32: the full 65 x 65 square
    "three": table(ref.rect_spans([(UNIT, 0), (12000, -9000), (0, UNIT)], ref.rect_of(4.0, 1.0, 1.0, 0.0), 7)),  # K = 3, one pair no unit vector
    "wide": table([[EMPTY_ROW] * 31 + [[-32, 31]] * 2 + [[-31, 32]] + [EMPTY_ROW] * 31]),  # K = 1, R = 32: 64-wide spans from either end of the range
}


@functools.lru_cache(maxsize=None)
def wanted(name, side, footprint, min_fit, outside_free):
    return ref.expected_footprint(ref.scene(name, side), FOOTPRINTS[footprint], min_fit, outside_free)


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
    """sentinel-filled destinations of one call: n planes of either output, each with a stride of its own and a few words behind, and the counts"""

    def __init__(self, n, mask_stride, fit_stride, slack=7):
        import torch

        self.n, self.mask_stride, self.fit_stride = n, mask_stride, fit_stride
        self.mask = torch.full((max(n * mask_stride + slack, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.fit = torch.full((max(n * fit_stride + slack, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.counts = torch.full((3 * max(n, 1) + 5,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

    def host(self):
        return dict(mask=self.mask.cpu().numpy(), fit=self.fit.cpu().numpy(), counts=self.counts.cpu().numpy())

    def all_sentinel(self):
        return all(bool((t == SIGNED_SENTINEL).all().item()) for t in (self.mask, self.fit, self.counts))


def raw_footprint(seg, n, dest, blocked, blocked_stride, spans, min_fit, outside_free=0, order=ROW, give=OUTPUTS, stream=None, own=False, **over):
    """gg_footprint_planes as the C ABI has it (blocked: a device tensor or an address, 0 = null; spans: [K, 2 R + 1, 2] or None); returns the
    status.  `over`: mask, fit, counts, mask_stride, fit_stride, n_headings, radius in place of what follows from the rest"""
    import torch

    def address(t):
        return (t.data_ptr() if torch.is_tensor(t) else t) or None

    x = _lib.GGPlaneFootprints()
    x.n, x.d_blocked, x.blocked_stride = n, address(blocked), blocked_stride
    host = None
    if spans is not None:
        host = np.ascontiguousarray(np.asarray(spans, np.int32))
        x.spans = host.ctypes.data_as(C.POINTER(C.c_int32))
        x.n_headings, x.radius = host.shape[0], host.shape[1] // 2
    x.n_headings, x.radius = over.get("n_headings", x.n_headings), over.get("radius", x.radius)
    x.min_fit, x.outside_free, x.order = min_fit, outside_free, order
    x.d_mask = address(over.get("mask", dest.mask if "mask" in give else 0))
    x.d_fit = address(over.get("fit", dest.fit if "fit" in give else 0))
    x.d_counts = address(over.get("counts", dest.counts if "counts" in give else 0))
    x.mask_stride, x.fit_stride = over.get("mask_stride", dest.mask_stride), over.get("fit_stride", dest.fit_stride)
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_footprint_planes(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check_map(host, i, want, dest, order, tag, give=OUTPUTS):
    """plane i of either output and row i of the counts of a downloaded Dest against footprint_ref.expected_footprint, and the words
    between a plane and its stride; an output that was not handed over holds its sentinels"""
    for name, stride in (("mask", dest.mask_stride), ("fit", dest.fit_stride)):
        words = host[name][i * stride: (i + 1) * stride]
        if name not in give:
            assert np.all(words == SIGNED_SENTINEL), f"{tag}: map {i}: {name} was not handed over and was written"
            continue
        plane = fusion_ref.lay(want[name].view(np.int32), ORDER[order]).ravel()
        bad = np.flatnonzero(words[: plane.size] != plane)
        assert len(bad) == 0, f"{tag}: map {i}: {len(bad)} words of {name} differ, first at {bad[0]}: {words[bad[0]]:#x} != {plane[bad[0]]:#x}"
        assert np.all(words[plane.size:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words between the {name} plane and its stride were written"
    got = host["counts"][3 * i: 3 * i + 3]
    if "counts" in give:
        assert got.tolist() == want["counts"].tolist(), f"{tag}: map {i}: counts {got.tolist()} != {want['counts'].tolist()}"
    else:
        assert np.all(got == SIGNED_SENTINEL), f"{tag}: map {i}: the counts were not handed over and were written"


def check_tail(host, dest, tag):
    assert np.all(host["mask"][dest.n * dest.mask_stride:] == SIGNED_SENTINEL), f"{tag}: the words behind the last mask plane were written"
    assert np.all(host["fit"][dest.n * dest.fit_stride:] == SIGNED_SENTINEL), f"{tag}: the words behind the last fit plane were written"
    assert np.all(host["counts"][3 * dest.n:] == SIGNED_SENTINEL), f"{tag}: the words behind the last counts were written"


def scene_buffer(names, side, order, stride):
    return pack([ref.scene(name, side) for name in names], ORDER[order], stride, slack=3)


# ---------------------------------------------------------------- 1. every scene, on bits

# (side, footprint, min_fit): 20 x 20 is one ragged tile, 67 x 67 four tiles of which three are ragged, 128 x 128 four whole tiles
CASES = [(67, "car", 32), (128, "car", 1), (128, "car", 20), (20, "small", 8), (67, "small", 1), (20, "gap", 6), (67, "gap", 8), (20, "cell", 1),
         (67, "cell in 3", 1), (20, "radius 0", 2), (128, "radius 0", 3), (20, "square", 1), (67, "square", 2), (67, "three", 1), (67, "three", 2),
         (128, "three", 3), (128, "wide", 1), (67, "wide", 1)]


@pytest.mark.parametrize("outside_free", [0, 1])
@pytest.mark.parametrize("order", [ROW, COL], ids=["row", "col"])
@pytest.mark.parametrize("side,footprint,min_fit", CASES)
def test_every_scene_on_bits(contexts, side, footprint, min_fit, order, outside_free):
    """all scenes as the maps of one call, every buffer with a stride of its own"""
    import torch

    seg = contexts(side)
    cells, n = side * side, len(SCENES)
    blocked_stride, mask_stride, fit_stride = cells + 3, cells + 8, cells + 1
    d_blocked = scene_buffer(SCENES, side, order, blocked_stride)
    before = d_blocked.clone()
    dst = Dest(n, mask_stride, fit_stride)
    spans = FOOTPRINTS[footprint]
    K = spans.shape[0]
    assert raw_footprint(seg, n, dst, d_blocked, blocked_stride, spans, min_fit, outside_free, order) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    host = dst.host()
    for i, name in enumerate(SCENES):
        check_map(host, i, wanted(name, side, footprint, min_fit, outside_free), dst, order, f"{name} {side} {footprint} min_fit={min_fit} {ORDER[order]} outside_free={outside_free}")
    check_tail(host, dst, "scenes")
    assert torch.equal(d_blocked, before)
    # what the scenes and the footprints are there for
    want = {name: wanted(name, side, footprint, min_fit, outside_free) for name in SCENES}
    assert all(np.all(w["mask"] >> np.uint32(K) == 0) if K < 32 else True for w in want.values())  # bits K .. 31 are zero
    if footprint in ("cell", "cell in 3"):  # the mask is "not blocked"
        for name in SCENES:
            assert np.array_equal(want[name]["mask"], (ref.scene(name, side) < 0).astype(np.uint32)), name
    if footprint == "square" and side == 20:  # larger than the map: with the outside blocked nothing fits, with it free only a map without a blocked cell
        for name in SCENES:
            fits_all = outside_free == 1 and not (ref.scene(name, side) >= 0).any()
            assert want[name]["counts"].tolist() == ([cells, cells, 0] if fits_all else [0, 0, cells]), name
        assert outside_free == 0 or want["free"]["counts"].tolist() == [cells, cells, 0]
    if footprint in ("gap", "radius 0"):  # an empty heading fits everywhere, also on a map that is all blocked
        empty = [k for k in range(K) if not ref.cells_of(spans, k)]
        assert empty and np.all(want["full"]["mask"] == sum(1 << k for k in empty))
    if footprint == "car" and side >= 67:
        p = want["random"]["p"]
        assert min((p == K).sum(), ((p > 0) & (p < K)).sum(), (p == 0).sum()) >= 10
    if side == 128:
        assert all((ref.scene("seams", side)[s] >= 0).any() and (ref.scene("seams", side)[:, s] >= 0).any() for s in ref.SEAMS)
    words = ref.scene("extremes", side)
    assert {ref.I32_MIN, -1, 0, ref.I32_MAX} == set(np.unique(words).tolist())


# ---------------------------------------------------------------- 2. each output alone and in pairs; equal strides

@pytest.mark.parametrize("order", [ROW, COL], ids=["row", "col"])
def test_each_output_alone_and_together(contexts, order):
    import torch

    side, footprint, min_fit = 67, "small", 3
    seg = contexts(side)
    cells, names = side * side, ("random", "rim", "seams")
    d_blocked = scene_buffer(names, side, order, cells)
    for give in (("mask",), ("fit",), ("counts",), ("mask", "fit"), ("mask", "counts"), ("fit", "counts"), OUTPUTS):
        for stride in (cells, cells + 5):
            dst = Dest(len(names), stride, stride)
            assert raw_footprint(seg, len(names), dst, d_blocked, cells, FOOTPRINTS[footprint], min_fit, 1, order, give=give) == 0, seg._L.gg_last_error(seg._ctx)
            torch.cuda.synchronize()
            host = dst.host()
            for i, name in enumerate(names):
                check_map(host, i, wanted(name, side, footprint, min_fit, 1), dst, order, f"{give} stride {stride}: {name}", give)
            check_tail(host, dst, str(give))
    one = Dest(1, cells, cells)  # one map
    assert raw_footprint(seg, 1, one, d_blocked, cells, FOOTPRINTS[footprint], min_fit, 0, order) == 0
    torch.cuda.synchronize()
    check_map(one.host(), 0, wanted("random", side, footprint, min_fit, 0), one, order, "n = 1")
    check_tail(one.host(), one, "n = 1")


# ---------------------------------------------------------------- 3. the ring, determinism, streams

def test_more_calls_than_the_ring_has_entries(contexts):
    """PARAM_RING + 3 calls back to back, each with a table of its own: an entry is reused only when its call has passed"""
    import torch

    side = 67
    seg = contexts(side)
    cells, names = side * side, ("random", "rim", "one")
    d_blocked = scene_buffer(names, side, ROW, cells)
    calls = []
    for j in range(PARAM_RING + 3):
        K = 2 + j
        spans = table(ref.rect_spans(ref.rotation_table([0.3 * j + 0.7 * k for k in range(K)]), ref.rect_of(1.0 + j, 0.5 * j, 1.0, 0.0, pad=0.4), 2 + j))
        calls.append((spans, 1 + j % K, Dest(3, cells, cells)))
    torch.cuda.synchronize()
    for spans, min_fit, dst in calls:
        assert raw_footprint(seg, 3, dst, d_blocked, cells, spans, min_fit, 1) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    for j, (spans, min_fit, dst) in enumerate(calls):
        host = dst.host()
        for i, name in enumerate(names):
            check_map(host, i, ref.expected_footprint(ref.scene(name, side), spans, min_fit, 1), dst, ROW, f"call {j}: {name}")
        check_tail(host, dst, f"call {j}")


def test_two_runs_byte_for_byte(contexts):
    import torch

    side = 128
    seg = contexts(side)
    cells, n = side * side, len(SCENES)
    d_blocked = scene_buffer(SCENES, side, COL, cells)
    runs = [Dest(n, cells, cells) for _ in range(2)]
    for dst in runs:
        assert raw_footprint(seg, n, dst, d_blocked, cells, FOOTPRINTS["car"], 4, 0, COL) == 0
    torch.cuda.synchronize()
    a, b = runs[0].host(), runs[1].host()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{key} differs between two runs"
    assert a["counts"][1] > 0


def test_on_a_caller_stream_and_on_the_contexts_own(contexts):
    import torch

    side, footprint, min_fit = 20, "small", 2
    seg = contexts(side)
    cells, names = side * side, ("random", "rim")
    d_blocked = scene_buffer(names, side, ROW, cells)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    mine, own = Dest(2, cells, cells), Dest(2, cells, cells)
    assert raw_footprint(seg, 2, mine, d_blocked, cells, FOOTPRINTS[footprint], min_fit, 1, stream=stream.cuda_stream) == 0
    stream.synchronize()
    assert raw_footprint(seg, 2, own, d_blocked, cells, FOOTPRINTS[footprint], min_fit, 1, own=True) == 0
    seg.synchronize()
    for dst, tag in ((mine, "caller stream"), (own, "own stream")):
        host = dst.host()
        for i, name in enumerate(names):
            check_map(host, i, wanted(name, side, footprint, min_fit, 1), dst, ROW, f"{tag}: {name}")
        check_tail(host, dst, tag)


# ---------------------------------------------------------------- 4. no map changes

def test_no_map_changes():
    """a context with two filtered maps and a fresh one: the lazy and fresh counters and an exported layer are the same before and after"""
    import torch

    side, K = 67, 3
    length, res = GEOMETRY[side]
    seg = api.GroundSegmentation().init(length, res, n_slots=K, max_points=MAX_POINTS)
    clouds = [scan_cloud(9400 + k, (0.0, 0.0)) for k in range(2)]
    pts, n_pts = batch_points(clouds, MAX_POINTS), [len(c) for c in clouds]
    seg.reset_maps(odom_z=0.1)
    seg.move_maps([(0.7, -0.4), (0.0, 0.4)], [POSE] * 2)
    seg.filter_batch(pts, n_pts, np.zeros((2, 3), np.float32), np.full(2, -1.73), slots=[0, 1])  # (map 2 stays fresh)
    assert lazy_count(seg) == 2 and fresh_count(seg) == 1
    layer_before = seg.export_layers(["ground"]).cpu().numpy()
    counters = (lazy_count(seg), fresh_count(seg))
    positions = [seg.map(s).getPosition() for s in range(K)]
    d_blocked = scene_buffer(("random", "rim", "one"), side, ROW, side * side)[: K * side * side].view(K, side, side)
    first = seg.footprint_planes(d_blocked, FOOTPRINTS["small"], min_fit=3, outside_free=True, on_torch_stream=True)
    seg.footprint_planes(d_blocked.transpose(1, 2).contiguous(), FOOTPRINTS["car"], order="col", on_torch_stream=True)
    assert (lazy_count(seg), fresh_count(seg)) == counters
    layer_after = seg.export_layers(["ground"]).cpu().numpy()
    torch.cuda.synchronize()
    assert (lazy_count(seg), fresh_count(seg)) == counters and positions == [seg.map(s).getPosition() for s in range(K)]
    assert same_bits(layer_before, layer_after) and np.isfinite(layer_before).any()
    assert first.counts.tolist() == [wanted(name, side, "small", 3, 1)["counts"].tolist() for name in ("random", "rim", "one")]
    seg.close()


# ---------------------------------------------------------------- 5. errors change nothing

def test_errors_change_nothing(contexts):
    import torch

    side, footprint, min_fit = 20, "small", 3
    seg = contexts(side, n_slots=5)
    cells, n = side * side, 3
    stride = cells + 8
    spans = FOOTPRINTS[footprint]
    K, R = spans.shape[0], spans.shape[1] // 2
    d_blocked = scene_buffer(("random", "rim", "one"), side, ROW, stride)
    before = d_blocked.clone()
    dst = Dest(n, stride, stride)
    fresh_before, lazy_before = fresh_count(seg), lazy_count(seg)

    def call(n=n, blocked=d_blocked, blocked_stride=stride, spans=spans, min_fit=min_fit, outside_free=0, order=ROW, **kw):
        return raw_footprint(seg, n, dst, blocked, blocked_stride, spans, min_fit, outside_free, order, **kw)

    def changed(k, a, row):
        t = spans.copy()
        t[k, a + R] = row
        return t

    x = _lib.GGPlaneFootprints()
    x.n = n
    assert seg._L.gg_footprint_planes(None, C.byref(x), None) == INVALID
    assert seg._L.gg_footprint_planes(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(blocked=0) == INVALID
    assert call(spans=None, n_headings=K, radius=R) == INVALID  # null spans
    assert call(give=()) == INVALID  # no output at all
    assert call(blocked_stride=cells - 1) == INVALID
    assert call(mask_stride=cells - 1) == INVALID
    assert call(fit_stride=cells - 1) == INVALID
    assert call(order=2) == INVALID
    assert call(order=-1) == INVALID
    for bad in (0, -1, 33):
        assert call(n_headings=bad) == INVALID, bad
    for bad in (-1, 33):
        assert call(radius=bad) == INVALID, bad
    for bad in (0, -3, K + 1):
        assert call(min_fit=bad) == INVALID, bad
    for bad in (-1, 2, 7):
        assert call(outside_free=bad) == INVALID, bad
    # a span beyond R, on either side; an empty row may hold anything
    assert call(spans=changed(0, 0, (-R - 1, 0))) == INVALID
    assert call(spans=changed(0, 0, (0, R + 1))) == INVALID
    assert call(spans=changed(0, 0, (ref.I32_MIN, ref.I32_MAX))) == INVALID
    # a table that is not column-convex: rows -1 and 1 hold column 0, row 0 does not
    hole = table([[[-1, 1], [1, 1], [-1, 1]]])
    assert not ref.valid_table(hole) and call(spans=hole, min_fit=1) == INVALID
    assert call(spans=table([[[0, 0], EMPTY_ROW, [0, 0]]]), min_fit=1) == INVALID
    assert call(n=6) == CAPACITY  # (more maps than the context has)
    # each pair of buffers that may not overlap: an output with the input, the outputs with each other
    last_cell = 4 * ((n - 1) * stride + cells - 1)
    for name in OUTPUTS:
        assert call(**{name: d_blocked}) == INVALID, name
        assert call(**{name: d_blocked.data_ptr() + last_cell}) == INVALID, name  # (the last cell of the last plane)
    assert call(mask=dst.fit) == INVALID and call(fit=dst.mask.data_ptr() + last_cell) == INVALID
    assert call(counts=dst.mask.data_ptr() + last_cell) == INVALID and call(counts=dst.fit) == INVALID
    assert call(mask=dst.counts.data_ptr() + 4 * (3 * n - 1)) == INVALID and call(fit=dst.counts) == INVALID  # (the last word of the last counts)
    assert call(n=0, blocked=0, spans=None, blocked_stride=0, order=9, min_fit=-4, outside_free=5, give=()) == 0  # n == 0: nothing to check
    torch.cuda.synchronize()
    assert dst.all_sentinel() and torch.equal(d_blocked, before)
    assert fresh_count(seg) == fresh_before and lazy_count(seg) == lazy_before
    # ... and the same arguments without a mistake are accepted, at the edges of the ranges too; the words behind an output belong to
    # the caller; without an output its stride is not looked at
    assert call() == 0, seg._L.gg_last_error(seg._ctx)
    assert call(min_fit=K, outside_free=1, order=COL) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(spans=changed(0, 2, (7, -9))) == 0, seg._L.gg_last_error(seg._ctx)  # (an empty row of any words)
    assert call(spans=changed(0, 0, (-R, R))) == 0, seg._L.gg_last_error(seg._ctx)
    assert call(give=("counts",), mask_stride=0, fit_stride=0) == 0, seg._L.gg_last_error(seg._ctx)
    both = torch.full((2 * n * cells + 3 * n + 2,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")  # mask planes, fit planes, counts, back to back
    assert call(mask=both, fit=both.data_ptr() + 4 * n * cells, counts=both.data_ptr() + 8 * n * cells, mask_stride=cells, fit_stride=cells) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert not dst.all_sentinel()
    got = both.cpu().numpy()
    assert np.all(got[: 2 * n * cells + 3 * n] != SIGNED_SENTINEL) and np.all(got[2 * n * cells + 3 * n:] == SIGNED_SENTINEL)
    for i, name in enumerate(("random", "rim", "one")):
        want = wanted(name, side, footprint, min_fit, 0)
        assert np.array_equal(got[i * cells: (i + 1) * cells], want["mask"].view(np.int32).ravel())
        assert np.array_equal(got[(n + i) * cells: (n + i + 1) * cells], want["fit"].ravel())
        assert got[2 * n * cells + 3 * i: 2 * n * cells + 3 * i + 3].tolist() == want["counts"].tolist()


# ---------------------------------------------------------------- 6. the chain on real data

def test_the_chain_from_a_drive(contexts):
    """three frames on two maps: move, filter, trace, fuse, then footprint_planes(fused state, min_fit=1) and route_planes(goals = the
    frontier, blocked = fit), every call on one stream; fit is held to footprint_ref and dist to route_ref on that plane"""
    import torch

    side, K = 67, 2
    seg = contexts(side, n_slots=K)
    seg.reset_maps(odom_z=0.0)
    track = np.array([[(0.0, 0.0), (0.0, 0.0)], [(1.1, -0.8), (-0.5, 0.4)], [(2.5, -0.9), (-1.9, 1.5)]])
    spans = api.footprint_spans(api.rotation_table([2.0 * np.pi * k / 8 for k in range(8)]), 2.0, 0.0, 0.5, 0.5, pad=0.3, radius=3)
    assert np.array_equal(spans, FOOTPRINTS["small"])
    evidence, outs, log = None, [api.FusionOutputs(), api.FusionOutputs()], []
    fuse = dict(hit=4, miss=3, free_threshold=-2, occ_threshold=4)  # (one miss makes a cell free: free cells from the first frame on)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for f in range(len(track)):
            shifts = seg.move_maps(track[f], [POSE] * K, on_torch_stream=True)
            clouds = [scan_cloud(9800 + 10 * f + k, track[f, k]) for k in range(K)]
            stride = stride_of(clouds)
            pts, n_pts = batch_points(clouds, stride), [len(c) for c in clouds]
            origins = np.concatenate([track[f], np.full((K, 1), 1.7)], axis=1).astype(np.float32)
            out = seg.filter_batch(pts, n_pts, origins, np.full(K, -1.73), want_masks=True)
            vis = seg.visibility_clouds(pts, n_pts, origins, masks=out.label_masks, min_height=0.2, max_height=3.0)
            fused = seg.fuse_states(vis.state, evidence, shifts=np.array(shifts), out=outs[f % 2], on_torch_stream=True, **fuse)
            evidence = fused.evidence
            fits = seg.footprint_planes(fused.state, spans, min_fit=1, outside_free=True, on_torch_stream=True)
            routes = seg.route_planes(fused.frontier, blocked=fits.fit, next=False, counts=False, on_torch_stream=True)
            log.append(dict(state=fused.state.clone(), frontier=fused.frontier.clone(), mask=fits.mask, fit=fits.fit, counts=fits.counts, dist=routes.dist))
    torch.cuda.synchronize()
    fitting = reached = 0
    for f, e in enumerate(log):
        for k in range(K):
            want = ref.expected_footprint(e["state"][k].cpu().numpy(), spans, 1, 1)
            assert np.array_equal(e["mask"][k].cpu().numpy().view(np.uint32), want["mask"]), f"frame {f}, map {k}"
            assert np.array_equal(e["fit"][k].cpu().numpy(), want["fit"]) and e["counts"][k].tolist() == want["counts"].tolist(), f"frame {f}, map {k}"
            route = route_ref.expected_routes(e["frontier"][k].cpu().numpy(), blocked=want["fit"])
            assert np.array_equal(e["dist"][k].cpu().numpy(), route["dist"]), f"frame {f}, map {k}"
            fitting += int(want["counts"][1])
            reached += int((route["dist"] != route_ref.NONE).sum())
    assert fitting > 100 and reached > 0


# ---------------------------------------------------------------- 7. the Python entry point

def test_python_entry_point(contexts):
    import torch

    side, names = 20, ("random", "rim", "one", "seams")
    n = len(names)
    seg = contexts(side)
    d_blocked = scene_buffer(names, side, ROW, side * side)[: n * side * side].view(n, side, side)
    spans = FOOTPRINTS["small"]
    K = spans.shape[0]
    a = seg.footprint_planes(d_blocked, spans, on_torch_stream=True)
    assert isinstance(a, api.FootprintOutputs)
    for t, shape in ((a.mask, (n, side, side)), (a.fit, (n, side, side)), (a.counts, (n, 3))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    b = seg.footprint_planes(d_blocked, spans.tolist(), min_fit=2, outside_free=True, mask=False, counts=False, on_torch_stream=True)
    assert b.mask is None and b.counts is None and tuple(b.fit.shape) == (n, side, side)
    c = seg.footprint_planes(d_blocked.transpose(1, 2).contiguous(), spans, min_fit=K, order="col", fit=False, on_torch_stream=True)
    again = seg.footprint_planes(d_blocked, spans, out=a)
    assert again is a
    seg.synchronize()
    torch.cuda.synchronize()
    for i, name in enumerate(names):
        want = wanted(name, side, "small", K, 0)  # min_fit=None means K
        assert np.array_equal(a.mask[i].cpu().numpy().view(np.uint32), want["mask"]) and np.array_equal(a.fit[i].cpu().numpy(), want["fit"]), name
        assert a.counts[i].tolist() == want["counts"].tolist() == c.counts[i].tolist(), name
        assert np.array_equal(c.mask[i].cpu().numpy().view(np.uint32), want["mask"].T), name
        assert np.array_equal(b.fit[i].cpu().numpy(), wanted(name, side, "small", 2, 1)["fit"]), name
    # bad arguments are refused before the call
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, out=api.FootprintOutputs(fit=d_blocked))
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, mask=False, out=a)  # (a mask that is not asked for)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, mask=False, fit=False, counts=False)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked.to(torch.int64), spans)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked[:, :, :19], spans)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans[:, :6])  # (an even number of rows)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, min_fit=K + 1)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, min_fit=0)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, outside_free=2)
    with pytest.raises(ValueError):
        seg.footprint_planes(d_blocked, spans, order="diagonal")
    with pytest.raises(api.GroundGridError):  # a span beyond R: the library's GG_ERR_INVALID
        bad = spans.copy()
        bad[0, 3] = (0, 4)
        seg.footprint_planes(d_blocked, bad)
    with pytest.raises(api.GroundGridError):  # more planes than the context has maps: the library's GG_ERR_CAPACITY
        seg.footprint_planes(torch.cat([d_blocked] * 3), spans)
