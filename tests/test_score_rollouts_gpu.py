"""gg_score_rollouts (the score of candidate trajectories of many maps over the heading mask, the cost plane, the clearance plane and the
cost-to-go volume, in device memory) on the device.  Expected values come from numpy and plain Python alone (tests/rollouts_ref.py, held
against records computed by hand by tests/test_score_rollouts_cpu.py).  Every comparison is on bits: every word of every record and of
d_best, the words between 8 P and the record stride and behind the last row, and the inputs after the call.  Every buffer has a stride of
its own.  The library's maps are square; the scenes are not their own transposes, so a swapped side or order shows all the same."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402
from tests import headings_ref  # noqa: E402
from tests import rollouts_ref as ref  # noqa: E402
from tests.test_export_layers_gpu import POSE, batch_points, fresh_count, same_bits, stride_of  # noqa: E402
from tests.test_fuse_states_gpu import MAX_POINTS, SIGNED_SENTINEL, scan_cloud  # noqa: E402
from tests.test_route_headings_gpu import GEOMETRY  # noqa: E402
from tests.test_split_clouds_gpu import PARAM_RING, lazy_count  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
REL, ABS = ref.RELATIVE, ref.ABSOLUTE
NONE = ref.NONE
NULLABLE = ("cost", "dist", "clear", "best")


@pytest.fixture(scope="module")
def contexts():
    """one context per (side, slots), made on demand and shared: no call of this file but the drive's changes a map"""
    made = {}

    def get(side, n_slots=8):
        if (side, n_slots) not in made:
            length, res = GEOMETRY[side]
            seg = api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=MAX_POINTS)
            assert seg.rows == seg.cols == side
            made[(side, n_slots)] = seg
        return made[(side, n_slots)]

    yield get
    for seg in made.values():
        seg.close()


def strided(rows, stride, slack):
    """host rows (1-d int32 arrays of one length) as one device buffer, row i at i * stride, sentinels between and behind"""
    import torch

    host = np.full(max(len(rows) * stride + slack, 1), SIGNED_SENTINEL, np.int32)
    for i, a in enumerate(rows):
        host[i * stride: i * stride + a.size] = a
    return torch.from_numpy(host).cuda()


class Scene:
    """the device buffers of one call, every one with a stride of its own, the outputs filled with sentinels, and the expectation"""

    def __init__(self, side, n, K, P, T, frame, order, shared, seed, reach=0, cost_max=252, table=None, starts=None, planes=None):
        import torch

        self.side, self.n, self.K, self.P, self.T, self.frame, self.order, self.reach, self.cost_max = side, n, K, P, T, frame, order, reach, cost_max
        cells = self.cells = side * side
        o = ORDER[order]
        self.rot = ref.rotations_of(K)
        self.masks, self.costs, self.clears, self.dists = planes if planes is not None else ref.random_planes(side, K, seed, n)
        self.table = table if table is not None else ref.mixed_table(P, T, K, side, seed, frame, None if shared else n)
        self.starts = np.asarray(starts if starts is not None else ref.sub_cell_starts(n, side, K, seed), np.int32)
        self.mask_stride, self.cost_stride, self.clear_stride, self.plane_stride = cells + 6, cells + 1, cells + 3, cells + 5
        self.dist_stride = K * self.plane_stride + 9
        self.table_stride = 0 if self.table.ndim == 3 else 4 * P * T + 13  # (odd: the tables of the odd maps are not 16-byte aligned)
        self.record_stride = 8 * P + 5
        self.d_mask = strided([ref.lay(m, o).ravel() for m in self.masks], self.mask_stride, 4)
        self.d_cost = strided([ref.lay(m, o).ravel() for m in self.costs], self.cost_stride, 2)
        self.d_clear = strided([ref.lay(m, o).ravel() for m in self.clears], self.clear_stride, 3)
        vols = []
        for d in self.dists:
            v = np.full(K * self.plane_stride, SIGNED_SENTINEL, np.int32)
            for k in range(K):
                v[k * self.plane_stride: k * self.plane_stride + cells] = ref.lay(d[k], o).ravel()
            vols.append(v)
        self.d_dist = strided(vols, self.dist_stride, 5)
        self.d_table = strided([self.table.ravel()] if self.table.ndim == 3 else [t.ravel() for t in self.table], self.table_stride or 4 * P * T, 8)
        self.records = torch.full((n * self.record_stride + 7,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.best = torch.full((4 * n + 3,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")
        self.inputs = [t.clone() for t in (self.d_mask, self.d_cost, self.d_clear, self.d_dist, self.d_table)]

    def want(self, give=NULLABLE):
        return ref.expected_rollouts(self.table, self.starts, self.K, self.frame, self.rot, self.masks, self.costs if "cost" in give else None,
                                     self.dists if "dist" in give else None, self.clears if "clear" in give else None, self.cost_max, self.reach, ORDER[self.order])

    def call(self, seg, give=NULLABLE, stream=None, own=False, **over):
        """gg_score_rollouts as the C ABI has it; `give`: the nullable buffers handed over; `over`: any field of the struct in place of what
        follows from the scene (a tensor, an address, 0 / None = null).  Returns the status"""
        import torch

        def address(t):
            return (t.data_ptr() if torch.is_tensor(t) else t) or None

        x = _lib.GGRollouts()
        x.n = over.get("n", self.n)
        x.d_mask, x.mask_stride = address(over.get("mask", self.d_mask)), over.get("mask_stride", self.mask_stride)
        x.d_cost, x.cost_stride = address(over.get("cost", self.d_cost if "cost" in give else 0)), over.get("cost_stride", self.cost_stride)
        x.d_dist = address(over.get("dist", self.d_dist if "dist" in give else 0))
        x.dist_stride, x.plane_stride = over.get("dist_stride", self.dist_stride), over.get("plane_stride", self.plane_stride)
        x.d_clear, x.clear_stride = address(over.get("clear", self.d_clear if "clear" in give else 0)), over.get("clear_stride", self.clear_stride)
        x.n_headings = over.get("n_headings", self.K)
        starts = over.get("starts", self.starts)
        keep = [None if starts is None else np.ascontiguousarray(np.asarray(starts, np.int32).reshape(-1, 3))]
        x.starts = keep[0].ctypes.data_as(C.POINTER(C.c_int32)) if keep[0] is not None else None
        rot = over.get("rotations", self.rot if self.frame == REL or over.get("frame") == REL else None)
        keep.append(None if rot is None else np.ascontiguousarray(np.asarray(rot, np.int32)))
        x.rotations = keep[1].ctypes.data_as(C.POINTER(C.c_int32)) if keep[1] is not None else None
        x.frame = over.get("frame", self.frame)
        x.d_table, x.table_stride = address(over.get("table", self.d_table)), over.get("table_stride", self.table_stride)
        x.n_rollouts, x.n_steps = over.get("n_rollouts", self.P), over.get("n_steps", self.T)
        x.cost_max, x.reach, x.order = over.get("cost_max", self.cost_max), over.get("reach", self.reach), over.get("order", self.order)
        x.d_records, x.record_stride = address(over.get("records", self.records)), over.get("record_stride", self.record_stride)
        x.d_best = address(over.get("best", self.best if "best" in give else 0))
        h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        return seg._L.gg_score_rollouts(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))

    def untouched(self):
        import torch

        return bool((self.records == SIGNED_SENTINEL).all().item()) and bool((self.best == SIGNED_SENTINEL).all().item()) and self.inputs_unchanged()

    def inputs_unchanged(self):
        import torch

        return all(torch.equal(a, b) for a, b in zip((self.d_mask, self.d_cost, self.d_clear, self.d_dist, self.d_table), self.inputs))

    def check(self, tag, give=NULLABLE, want=None):
        """the downloaded outputs against the reference: every record word, the words between 8 P and the stride and behind the last row,
        d_best or its sentinels, and the inputs as they were"""
        want = want if want is not None else self.want(give)
        rec, best = self.records.cpu().numpy(), self.best.cpu().numpy()
        for i in range(self.n):
            row = rec[i * self.record_stride: (i + 1) * self.record_stride]
            got = row[: 8 * self.P].reshape(self.P, 8)
            bad = np.flatnonzero((got != want["records"][i]).any(axis=1))
            assert len(bad) == 0, f"{tag}: map {i}: {len(bad)} records differ, first {bad[0]}: {got[bad[0]].tolist()} != {want['records'][i][bad[0]].tolist()}"
            assert np.all(row[8 * self.P:] == SIGNED_SENTINEL), f"{tag}: map {i}: the words between the records and the stride were written"
        assert np.all(rec[self.n * self.record_stride:] == SIGNED_SENTINEL), f"{tag}: the words behind the last row of records were written"
        if "best" in give:
            assert np.array_equal(best[: 4 * self.n].reshape(self.n, 4), want["best"]), f"{tag}: best {best[: 4 * self.n].tolist()} != {want['best'].tolist()}"
        else:
            assert np.all(best[: 4 * self.n] == SIGNED_SENTINEL), f"{tag}: d_best was not handed over and was written"
        assert np.all(best[4 * self.n:] == SIGNED_SENTINEL), f"{tag}: the words behind d_best were written"
        assert self.inputs_unchanged(), f"{tag}: an input changed"
        return want


def run(seg, tag, *args, give=NULLABLE, **kw):
    import torch

    call_kw = {k: kw.pop(k) for k in ("stream", "own") if k in kw}
    sc = Scene(seg.rows, *args, **kw)
    rc = sc.call(seg, give, **call_kw)
    assert rc == 0, f"{tag}: {seg._L.gg_last_error(seg._ctx)}"
    if call_kw.get("own"):
        seg.synchronize()
    torch.cuda.synchronize()
    return sc, sc.check(tag, give)


# ---------------------------------------------------------------- 1. the scenes of one call, on bits

# side, n, K, P, T, frame, order, shared table, reach: every side, K, P, T and reach of the list at least once, both orders and frames, shared
# and per-map tables; P * T is kept small enough for the plain loops of the reference
CASES = [(20, 3, 8, 63, 33, REL, ROW, True, 0), (20, 2, 1, 1, 1, ABS, COL, False, 1), (23, 3, 32, 64, 2, ABS, ROW, False, 5), (23, 2, 8, 65, 128, REL, COL, True, 63),
         (41, 2, 32, 1023, 2, REL, COL, False, 0), (41, 3, 1, 1025, 33, REL, ROW, True, 5), (67, 2, 8, 2049, 2, ABS, ROW, True, 0), (67, 3, 32, 65, 33, REL, COL, False, 1),
         (67, 2, 8, 1, 128, ABS, COL, True, 63), (41, 2, 8, 2049, 33, REL, ROW, True, 5), (20, 4, 8, 1025, 1, ABS, ROW, False, 0)]


@pytest.mark.parametrize("side,n,K,P,T,frame,order,shared,reach", CASES)
def test_scenes_of_one_call(contexts, side, n, K, P, T, frame, order, shared, reach):
    sc, want = run(contexts(side), f"{side} n={n} K={K} P={P} T={T} frame={frame} {ORDER[order]} reach={reach}", n, K, P, T, frame, order, shared, side + P + T, reach=reach)
    rec = want["records"]
    if P * T >= 64:
        assert (rec[..., 0] > 0).any() and (rec[..., 0] < rec[..., 1]).any()


def test_a_map_without_a_start_among_maps_with_one_and_n_one(contexts):
    seg = contexts(23)
    starts = ref.sub_cell_starts(3, 23, 8, 4)
    starts[1] = (-1, -77, 99)  # (the other two words are not looked at)
    sc, want = run(seg, "no start", 3, 8, 65, 5, REL, ROW, True, 11, starts=starts)
    assert want["records"][1].tolist() == [list(ref.NO_START)] * 65 and want["best"][1].tolist() == [-1, NONE, 0, 0]
    run(seg, "n = 1", 1, 8, 65, 5, REL, COL, False, 12)
    run(seg, "n = 1 without a start", 1, 8, 1025, 2, ABS, COL, True, 13, starts=[(-1, 0, 0)])
    # the corners of the start range
    run(seg, "corner starts", 2, 8, 64, 3, REL, ROW, True, 14, starts=[(0, 0, 0), (16 * 23 - 1, 16 * 23 - 1, 7)])


@pytest.mark.parametrize("frame,shared", [(REL, True), (ABS, False)])
def test_the_garbage_table(contexts, frame, shared):
    """extreme words in every field (INT32_MIN, INT32_MAX, their neighbours, powers of two, random words): GG_OK, the reference's records,
    nothing outside the outputs changed"""
    side, n, K, P, T = 41, 3, 32, 1025, 6
    table = ref.garbage_table(P, T, 5 + frame, None if shared else n)
    sc, want = run(contexts(side), "garbage", n, K, P, T, frame, ROW, shared, 21, table=table)
    assert (want["records"][..., 0] > 0).any()
    sc, want = run(contexts(side), "garbage col, reach", n, K, P, T, frame, COL, shared, 22, table=table, reach=63)


# ---------------------------------------------------------------- 2. the identity with gg_route_headings

@pytest.mark.parametrize("side,K,order", [(41, 8, ROW), (67, 16, COL)])
def test_rollouts_along_the_next_chain_total_the_cost_to_go(contexts, side, K, order):
    """D and d_next of gg_route_headings on a scene with a cost plane.  From a reached start the absolute-frame rollout made of the first j
    moves of the d_next chain (s the move's, the same cost_max) has total == D(start) exactly, for every j from 0 (the empty rollout) to
    the whole chain; rollouts made of other admissible moves (random walks) have total >= D(start) or none; d_best holds D(start) and
    the smallest p that attains it.  The walks come first in the table, so the best p is a walk only where the walk is optimal itself."""
    import torch

    seg = contexts(side)
    o = ORDER[order]
    mask, goals, cost, _ = headings_ref.random_scene(side, K, 500 + side)
    moves = headings_ref.table(K, 1, 10, turn=3, reverse_pct=150)
    lay = lambda a: torch.from_numpy(ref.lay(a, o)[None].copy()).cuda()
    routes = seg.route_headings(lay(mask), lay(goals), moves, lay(cost), order=o, on_torch_stream=True)
    torch.cuda.synchronize()
    D = routes.dist[0].cpu().numpy()
    nxt = routes.next[0].cpu().numpy()
    if o == "col":
        D, nxt = D.transpose(0, 2, 1), nxt.transpose(0, 2, 1)
    words = mask.view(np.uint32)

    def chain_from(k, r, c):
        out = []
        while nxt[k, r, c] != _lib.GG_HEADINGS_AT_GOAL and len(out) <= 128:
            da, db, k2, s = (int(v) for v in moves[k, nxt[k, r, c]])
            r, c, k = r + da, c + db, k2
            out.append((16 * r + 8, 16 * c + 8, k, s))
        return out

    reached = np.argwhere((D != NONE) & (D > 0))
    rng = np.random.default_rng(side)
    chain, start = None, None
    for k, r, c in reached[rng.permutation(len(reached))]:
        got = chain_from(int(k), int(r), int(c))
        if 12 <= len(got) <= 100:
            chain, start = got, (int(k), int(r), int(c))
            break
    assert chain is not None
    k0, r0, c0 = start
    L = len(chain)
    walks = []
    for _ in range(40):
        k, r, c, walk = k0, r0, c0, []
        for _ in range(int(rng.integers(1, L + 1))):
            ok = [m for m in moves[k] if m[3] > 0 and 0 <= r + m[0] < side and 0 <= c + m[1] < side and (int(words[r + m[0], c + m[1]]) >> int(m[2])) & 1]
            if not ok:
                break
            da, db, k, s = (int(v) for v in ok[int(rng.integers(len(ok)))])
            r, c = r + da, c + db
            walk.append((16 * r + 8, 16 * c + 8, k, s))
        walks.append(walk)
    rollouts = walks + [chain[:j] for j in range(L + 1)]
    P, T = len(rollouts), L
    table = np.zeros((T, P, 4), np.int32)
    for p, poses in enumerate(rollouts):
        for t, e in enumerate(poses):
            table[t, p] = e
    planes = (mask[None], cost[None], np.zeros((1, side, side), np.int32), D[None])
    sc = Scene(side, 1, K, P, T, ABS, order, True, 0, table=table, starts=[(16 * r0 + 8, 16 * c0 + 8, k0)], planes=planes)
    assert sc.call(seg) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    sc.check("chain")
    rec = sc.records.cpu().numpy()[: 8 * P].reshape(P, 8)
    d0 = int(D[k0, r0, c0])
    assert (rec[len(walks):, 7] == d0).all() and (rec[len(walks):, 0] == np.arange(L + 1)).all()
    assert (rec[: len(walks), 0] == rec[: len(walks), 1]).all() and (rec[: len(walks), 7] >= d0).all()  # (complete by construction)
    best = sc.best.cpu().numpy()[:4]
    assert best[1] == d0 and best[0] == np.flatnonzero(rec[:, 7] == d0)[0] and rec[best[0], 7] == d0 and best[2] == P


def test_relative_frame_equals_absolute_frame_on_the_rotated_poses(contexts):
    import torch

    side, n, K, P, T = 41, 3, 8, 257, 9
    seg = contexts(side)
    rel = Scene(side, n, K, P, T, REL, ROW, False, 31)
    poses = np.zeros_like(rel.table)
    for i in range(n):
        for t in range(T):
            for p in range(P):
                poses[i, t, p, :3] = ref.pose(rel.table[i, t, p], rel.starts[i], K, REL, rel.rot)
    poses[..., 3] = rel.table[..., 3]
    absolute = Scene(side, n, K, P, T, ABS, ROW, False, 31, table=poses, starts=rel.starts, planes=(rel.masks, rel.costs, rel.clears, rel.dists))
    assert rel.call(seg) == 0 and absolute.call(seg) == 0
    torch.cuda.synchronize()
    rel.check("relative")
    absolute.check("absolute")
    assert torch.equal(rel.records, absolute.records) and torch.equal(rel.best, absolute.best)


# ---------------------------------------------------------------- 3. the nullable buffers, the ring, determinism, the streams

def test_every_subset_of_the_nullable_buffers(contexts):
    seg = contexts(20)
    for r in range(len(NULLABLE) + 1):
        for give in itertools.combinations(NULLABLE, r):
            run(seg, f"give {give}", 2, 8, 65, 5, REL if r % 2 else ABS, ROW if len(give) % 2 else COL, bool(r % 2), 40 + r, give=give)


def test_more_calls_than_the_ring_has_entries_and_two_runs(contexts):
    """PARAM_RING + 3 calls back to back, each with a table, starts and a frame of its own, nothing synchronised in between: every call's
    outputs are its own; the whole sequence again gives the same bytes"""
    import torch

    seg = contexts(23)
    runs = []
    for _ in range(2):
        scenes = [Scene(23, 3, 8, 65 + j, 4, REL if j % 2 else ABS, ROW, bool(j % 3), 50 + j) for j in range(PARAM_RING + 3)]
        for sc in scenes:
            assert sc.call(seg) == 0
        torch.cuda.synchronize()
        for j, sc in enumerate(scenes):
            sc.check(f"call {j}")
        runs.append([(sc.records.cpu().numpy().tobytes(), sc.best.cpu().numpy().tobytes()) for sc in scenes])
    assert runs[0] == runs[1]


def test_a_callers_stream_and_the_contexts_own(contexts):
    import torch

    seg = contexts(41)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        run(seg, "caller stream", 2, 8, 257, 5, REL, ROW, True, 60, stream=stream.cuda_stream)
    run(seg, "own stream", 2, 8, 257, 5, ABS, COL, False, 61, own=True)


# ---------------------------------------------------------------- 4. no map changes

def test_no_map_changes():
    """a context with two filtered maps and a fresh one: the lazy and fresh counters, the positions and an exported layer are the same
    before and after"""
    import torch

    side, n = 67, 3
    length, res = GEOMETRY[side]
    seg = api.GroundSegmentation().init(length, res, n_slots=n, max_points=MAX_POINTS)
    clouds = [scan_cloud(9400 + k, (0.0, 0.0)) for k in range(2)]
    pts, n_pts = batch_points(clouds, MAX_POINTS), [len(c) for c in clouds]
    seg.reset_maps(odom_z=0.1)
    seg.move_maps([(0.7, -0.4), (0.0, 0.4)], [POSE] * 2)
    seg.filter_batch(pts, n_pts, np.zeros((2, 3), np.float32), np.full(2, -1.73), slots=[0, 1])  # (map 2 stays fresh)
    assert lazy_count(seg) == 2 and fresh_count(seg) == 1
    layer_before = seg.export_layers(["ground"]).cpu().numpy()
    counters = (lazy_count(seg), fresh_count(seg))
    positions = [seg.map(s).getPosition() for s in range(n)]
    first, want = run(seg, "no map changes", n, 8, 257, 6, REL, ROW, True, 70)
    run(seg, "no map changes, col", n, 8, 65, 6, ABS, COL, False, 71)
    assert (lazy_count(seg), fresh_count(seg)) == counters
    layer_after = seg.export_layers(["ground"]).cpu().numpy()
    torch.cuda.synchronize()
    assert (lazy_count(seg), fresh_count(seg)) == counters and positions == [seg.map(s).getPosition() for s in range(n)]
    assert same_bits(layer_before, layer_after) and np.isfinite(layer_before).any()
    seg.close()


# ---------------------------------------------------------------- 5. errors change nothing

def test_errors_change_nothing(contexts):
    import torch

    side, K, n, P, T = 20, 8, 3, 65, 4
    seg = contexts(side, n_slots=5)
    cells = side * side
    sc = Scene(side, n, K, P, T, REL, ROW, False, 80)
    fresh_before, lazy_before = fresh_count(seg), lazy_count(seg)
    call = lambda **kw: sc.call(seg, **kw)
    x = _lib.GGRollouts()
    x.n = n
    assert seg._L.gg_score_rollouts(None, C.byref(x), None) == INVALID
    assert seg._L.gg_score_rollouts(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(mask=0) == INVALID and call(table=0) == INVALID and call(records=0) == INVALID and call(starts=None) == INVALID
    assert call(rotations=None, frame=REL) == INVALID
    for bad in (0, -1, 33):
        assert call(n_headings=bad) == INVALID, bad
    for bad in (0, -1, 65537):
        assert call(n_rollouts=bad, table_stride=0) == INVALID, bad
    for bad in (0, -1, 129):
        assert call(n_steps=bad, table_stride=0) == INVALID, bad
    assert call(frame=2) == INVALID and call(frame=-1) == INVALID and call(order=2) == INVALID and call(order=-1) == INVALID
    assert call(reach=-1) == INVALID and call(reach=64) == INVALID
    assert call(mask_stride=cells - 1) == INVALID and call(cost_stride=cells - 1) == INVALID and call(clear_stride=cells - 1) == INVALID
    assert call(plane_stride=cells - 1) == INVALID and call(dist_stride=K * sc.plane_stride - 1) == INVALID
    assert call(record_stride=8 * P - 1) == INVALID
    assert call(table_stride=4 * P * T - 1) == INVALID and call(table_stride=1) == INVALID
    for word in (16385, -16385, 2 ** 31 - 1, -2 ** 31):
        rot = sc.rot.copy()
        rot[K - 1, 1] = word
        assert call(rotations=rot) == INVALID, word
    good = sc.starts.tolist()
    for bad in ((-2, 8, 0), (16 * side, 8, 0), (8, -1, 0), (8, 16 * side, 0), (8, 8, K), (8, 8, -1), (-2 ** 31, 8, 0)):
        assert call(starts=[good[0], bad, good[2]]) == INVALID, bad
    # the limit T * 32767 * cost_max <= 2^31 - 2 at its edge
    at_limit = (2 ** 31 - 2) // (T * 32767)
    assert call(cost_max=0) == INVALID and call(cost_max=-5) == INVALID and call(cost_max=at_limit + 1) == INVALID and call(cost_max=2 ** 31 - 1) == INVALID
    assert call(n=6) == CAPACITY  # (more maps than the context has)
    # each pair of buffers that may not overlap: an output with every input (its first word and the last word the call reads), the outputs
    # with each other
    last_in = {"mask": 4 * ((n - 1) * sc.mask_stride + cells - 1), "cost": 4 * ((n - 1) * sc.cost_stride + cells - 1), "clear": 4 * ((n - 1) * sc.clear_stride + cells - 1),
               "dist": 4 * ((n - 1) * sc.dist_stride + (K - 1) * sc.plane_stride + cells - 1), "table": 4 * ((n - 1) * sc.table_stride + 4 * P * T - 1)}
    last_out = {"records": 4 * ((n - 1) * sc.record_stride + 8 * P - 1), "best": 4 * (4 * n - 1)}
    sources = {"mask": sc.d_mask, "cost": sc.d_cost, "clear": sc.d_clear, "dist": sc.d_dist, "table": sc.d_table}
    for name in ("records", "best"):
        for src, t in sources.items():
            assert call(**{name: t}) == INVALID, (name, src)
            assert call(**{name: t.data_ptr() + last_in[src]}) == INVALID, (name, src)
    assert call(records=sc.best.data_ptr() + last_out["best"]) == INVALID and call(best=sc.records.data_ptr() + last_out["records"]) == INVALID
    assert call(records=sc.best) == INVALID and call(best=sc.records) == INVALID
    assert call(n=0, mask=0, table=0, records=0, starts=None, order=9, frame=7, cost_max=-4, n_headings=99, n_rollouts=0, n_steps=0, reach=-3) == 0  # n == 0: nothing to check
    torch.cuda.synchronize()
    assert sc.untouched()
    assert fresh_count(seg) == fresh_before and lazy_count(seg) == lazy_before
    # ... and the same arguments without the mistake are accepted, at the edges of the ranges too
    assert call() == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    sc.check("accepted")
    edge = Scene(side, n, K, P, T, REL, COL, False, 81, cost_max=at_limit, reach=63, starts=[(0, 0, 0), (16 * side - 1, 16 * side - 1, K - 1), (-1, 5, 5)])
    assert edge.call(seg) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    edge.check("at the limit")
    bare = Scene(side, n, K, P, T, ABS, ROW, True, 82)
    assert bare.call(seg, give=(), rotations=None, cost_stride=0, clear_stride=0, dist_stride=0, plane_stride=0) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    bare.check("nothing nullable", give=())


# ---------------------------------------------------------------- 6. the Python entry point

def test_python_entry_point(contexts):
    import torch

    side, n, K, P, T = 23, 3, 8, 65, 7
    seg = contexts(side)
    rot = ref.rotations_of(K)
    masks, costs, clears, dists = ref.random_planes(side, K, 90, n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_mask, d_cost, d_clear, d_dist = dev(masks), dev(costs), dev(clears), dev(dists)
    major = ref.mixed_table(P, T, K, side, 91, REL)            # [T, P, 4]
    lib_table = dev(major.transpose(1, 0, 2))                  # [P, T, 4]
    starts = ref.sub_cell_starts(n, side, K, 92)
    want = ref.expected_rollouts(major, starts, K, REL, rot, masks, costs, dists, clears, reach=7)
    a = seg.score_rollouts(d_mask, lib_table, starts, rotations=rot, cost=d_cost, dist=d_dist, clear=d_clear, reach=7, on_torch_stream=True)
    assert isinstance(a, api.RolloutOutputs)
    for t, shape in ((a.records, (n, P, 8)), (a.best, (n, 4))):
        assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    b = seg.score_rollouts(d_mask, dev(major), starts.tolist(), rotations=rot.tolist(), cost=d_cost, dist=d_dist, clear=d_clear, reach=7, step_major=True,
                           best=False, on_torch_stream=True)
    assert b.best is None
    # per-map tables, the absolute frame (K from dist), column-major planes, the context's own stream
    per_map = ref.mixed_table(P, T, K, side, 93, ABS, n)      # [n, T, P, 4]
    tr = [t.transpose(-1, -2).contiguous() for t in (d_mask, d_cost, d_clear, d_dist)]
    c = seg.score_rollouts(tr[0], dev(per_map.transpose(0, 2, 1, 3)), starts, relative=False, cost=tr[1], dist=tr[3], clear=tr[2], order="col")
    want_c = ref.expected_rollouts(per_map, starts, K, ABS, None, masks, costs, dists, clears, order="col")
    again = seg.score_rollouts(d_mask, lib_table, starts, rotations=rot, cost=d_cost, dist=d_dist, clear=d_clear, reach=7, out=a, on_torch_stream=True)
    assert again is a
    seg.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(a.records.cpu().numpy(), want["records"]) and np.array_equal(a.best.cpu().numpy(), want["best"])
    assert np.array_equal(b.records.cpu().numpy(), want["records"])
    assert np.array_equal(c.records.cpu().numpy(), want_c["records"]) and np.array_equal(c.best.cpu().numpy(), want_c["best"])
    view = a.table(1)
    assert view.dtype == api.ROLLOUT_DTYPE and view.shape == (P,) and np.array_equal(view["total"], want["records"][1][:, 7])
    # bad arguments are refused before the call
    ok = dict(rotations=rot, cost=d_cost, dist=d_dist, clear=d_clear)
    bad_calls = [dict(order="diagonal"), dict(reach=64), dict(reach=-1), dict(cost_max=0), dict(cost_max=2 ** 31 - 1), dict(rotations=None),
                 dict(rotations=rot[:4]), dict(rotations=rot * 2), dict(cost=d_cost[:, :, :19]), dict(clear=d_clear.to(torch.int64)), dict(dist=d_dist[:, :4].contiguous()),
                 dict(out=api.RolloutOutputs(records=torch.zeros((n, P, 8), dtype=torch.int32, device="cuda"), best=d_mask)), dict(best=False, out=a),
                 dict(out=api.RolloutOutputs(records=torch.zeros((n, P + 1, 8), dtype=torch.int32, device="cuda")))]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            seg.score_rollouts(d_mask, lib_table, starts, **{**ok, **kw})
    for bad_starts in (starts[:2], [(-2, 8, 0)] * n, [(8, 16 * side, 0)] * n, [(8, 8, K)] * n, np.zeros((n, 2), np.int32)):
        with pytest.raises(ValueError):
            seg.score_rollouts(d_mask, lib_table, bad_starts, **ok)
    for bad_table in (lib_table.to(torch.int64), lib_table[:, :, :3], lib_table.cpu(), dev(per_map[:2]), torch.zeros((2, 129, 4), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            seg.score_rollouts(d_mask, bad_table, starts, **ok)
    with pytest.raises(ValueError):
        seg.score_rollouts(d_mask, lib_table.transpose(0, 1), starts, step_major=True, **ok)  # (a step-major table must be contiguous)
    with pytest.raises(ValueError):
        seg.score_rollouts(d_mask, lib_table, starts, relative=False)  # (nothing tells K)
    with pytest.raises(api.GroundGridError):  # more planes than the context has maps: the library's GG_ERR_CAPACITY
        seg.score_rollouts(torch.cat([d_mask] * 3), lib_table, np.concatenate([starts] * 3), rotations=rot)


# ---------------------------------------------------------------- 7. the chain on real data

def test_the_chain_from_a_drive(contexts):
    """three frames on two maps: move, filter, trace, fuse, footprint_planes, route_headings, then score_rollouts with the arc library of
    rollout_arcs from the robot cell, every call on one stream; every record is held to the reference on the downloaded planes"""
    import torch

    side, n, K = 67, 2, 8
    seg = contexts(side, n_slots=n)
    seg.reset_maps(odom_z=0.0)
    track = np.array([[(0.0, 0.0), (0.0, 0.0)], [(1.1, -0.8), (-0.5, 0.4)], [(2.5, -0.9), (-1.9, 1.5)]])
    rotations = api.rotation_table([2.0 * np.pi * k / K for k in range(K)])
    spans = api.footprint_spans(rotations, 2.0, 0.0, 0.5, 0.5, pad=0.3, radius=3)
    moves = api.heading_moves(rotations, step=1, unit=10, turn=3, reverse_pct=200)
    arcs = api.rollout_arcs(rotations, [0.5, 1.0, 1.5], np.linspace(-0.3, 0.3, 21), 12, unit=10)  # [63, 12, 4]
    evidence, outs, log = None, [api.FusionOutputs(), api.FusionOutputs()], []
    fuse = dict(hit=4, miss=3, free_threshold=-2, occ_threshold=4)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        d_arcs = torch.from_numpy(arcs).cuda()
        for f in range(len(track)):
            shifts = seg.move_maps(track[f], [POSE] * n, on_torch_stream=True)
            clouds = [scan_cloud(9800 + 10 * f + k, track[f, k]) for k in range(n)]
            stride = stride_of(clouds)
            pts, n_pts = batch_points(clouds, stride), [len(c) for c in clouds]
            origins = np.concatenate([track[f], np.full((n, 1), 1.7)], axis=1).astype(np.float32)
            out = seg.filter_batch(pts, n_pts, origins, np.full(n, -1.73), want_masks=True)
            vis = seg.visibility_clouds(pts, n_pts, origins, masks=out.label_masks, min_height=0.2, max_height=3.0)
            fused = seg.fuse_states(vis.state, evidence, shifts=np.array(shifts), out=outs[f % 2], on_torch_stream=True, **fuse)
            evidence = fused.evidence
            fits = seg.footprint_planes(fused.state, spans, min_fit=1, outside_free=True, fit=False, counts=False, on_torch_stream=True)
            routes = seg.route_headings(fits.mask, fused.frontier, moves, on_torch_stream=True)
            starts = [(16 * (side // 2) + 8, 16 * (side // 2) + 8, f % K)] * n
            scores = seg.score_rollouts(fits.mask, d_arcs, starts, rotations=rotations, dist=routes.dist, reach=20, on_torch_stream=True)
            log.append(dict(mask=fits.mask, dist=routes.dist, scores=scores, starts=starts))
    torch.cuda.synchronize()
    scored = 0
    for f, e in enumerate(log):
        want = ref.expected_rollouts(arcs.transpose(1, 0, 2), e["starts"], K, REL, rotations, e["mask"].cpu().numpy(), None, e["dist"].cpu().numpy(), None, reach=20)
        assert np.array_equal(e["scores"].records.cpu().numpy(), want["records"]), f"frame {f}"
        assert np.array_equal(e["scores"].best.cpu().numpy(), want["best"]), f"frame {f}"
        scored += int(want["best"][:, 3].sum())
    assert scored > 0


# ---------------------------------------------------------------- 8. one map of the size of the benchmark's

def test_a_map_of_364_cells_a_side():
    import torch

    side, K, P, T = 364, 16, 2048, 32
    length, res = GEOMETRY[side]
    seg = api.GroundSegmentation().init(length, res, n_slots=1, max_points=MAX_POINTS)
    assert seg.rows == seg.cols == side
    rot = api.rotation_table(2.0 * np.pi * np.arange(K) / K)
    arcs = api.rollout_arcs(rot, np.linspace(0.5, 4.0, 32), np.linspace(-0.2, 0.2, 64), T)
    assert arcs.shape == (P, T, 4)
    planes = ref.random_planes(side, K, 364, 1, blocked=0.01)
    sc = Scene(side, 1, K, P, T, REL, ROW, True, 0, table=np.ascontiguousarray(arcs.transpose(1, 0, 2)), starts=[(16 * 182 + 8, 16 * 182 + 8, 3)], planes=planes)
    sc.rot = rot
    assert sc.call(seg) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    want = sc.check("364")
    assert (want["records"][0][:, 0] == T).sum() > 100 and want["best"][0, 3] > 50
    seg.close()
