"""gg_track_clusters (this scan's clusters of many maps associated with the last scan's, in device memory, one launch) on the device.
Expected values come from numpy alone (tests/tracks_ref.py, held together by tests/test_track_clusters_cpu.py).  Every comparison is on
bits: every record below the cluster count, the four head words, every cell of the track plane; and the records from the count on, the
words between rows * cols and the stride and the words behind the last plane keep their sentinel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402
from tests import tracks_ref  # noqa: E402
from tests.test_export_layers_gpu import POSE, SENTINEL, batch_points, stride_of  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, GEOMETRY_ERR, CAPACITY = -1, -2, -5
ROW, COL = _lib.GG_PLANES_ROWMAJOR, _lib.GG_PLANES_COLMAJOR
ORDER = {ROW: "row", COL: "col"}
SIGNED_SENTINEL = SENTINEL - (1 << 32) if SENTINEL >= (1 << 31) else SENTINEL
GEOMETRY = {23: (8.0, 0.348), 41: (14.0, 0.3415)}  # side: (length, resolution)
N_SLOTS = 5


# ---------------------------------------------------------------- helpers

@pytest.fixture(scope="module")
def contexts():
    """one context per side, made on demand and shared: no call of this file changes a map"""
    made = {}

    def get(side):
        if side not in made:
            length, res = GEOMETRY[side]
            seg = api.GroundSegmentation().init(length, res, n_slots=N_SLOTS, max_points=1024)
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

    host = np.full(max(len(planes) * stride + slack, 1), SIGNED_SENTINEL, np.int32)
    for i, a in enumerate(planes):
        host[i * stride: i * stride + a.size] = lay(np.asarray(a, np.int32), order).ravel()
    return torch.from_numpy(host).cuda()


def upload(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


class Dest:
    """sentinel-filled destinations of one call"""

    FIELDS = ("tracks", "heads", "plane")

    def __init__(self, n, M, plane_stride, slack=0):
        import torch

        def full(count):
            return torch.full((max(count, 1),), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

        self.n, self.M, self.plane_stride = n, M, plane_stride
        self.tracks, self.heads, self.plane = full(n * M * 8 + 5), full(4 * n + 3), full(n * plane_stride + slack)

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}

    def all_sentinel(self):
        return all(bool((getattr(self, k) == SIGNED_SENTINEL).all().item()) for k in self.FIELDS)


def raw_track(seg, n, dest, cells, cells_stride, prev=None, prev_stride=0, tracks_in=None, heads_in=None, shifts=None, M=256, g=1, order=ROW,
              give_plane=True, **over):
    """gg_track_clusters as the C ABI has it (device tensors or addresses, 0 / None = null); returns the status.  `over`: tracks_out,
    heads_out, cell_track, track_stride in place of `dest`'s"""
    import torch

    def address(t):
        return (t.data_ptr() if torch.is_tensor(t) else t) or None

    x = _lib.GGClusterTracks()
    x.n, x.d_cells, x.cells_stride = n, address(cells), cells_stride
    x.d_cells_prev, x.prev_stride, x.d_tracks_in, x.d_heads_in = address(prev), prev_stride, address(tracks_in), address(heads_in)
    sh = None
    if shifts is not None:
        sh = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32).reshape(-1, 2))
        x.shifts = sh.ctypes.data_as(C.POINTER(C.c_int32))
    x.max_clusters, x.gate, x.order = M, g, order
    x.d_tracks_out = address(over.get("tracks_out", dest.tracks))
    x.d_heads_out = address(over.get("heads_out", dest.heads))
    x.d_cell_track = address(over.get("cell_track", dest.plane if give_plane else 0))
    x.track_stride = over.get("track_stride", dest.plane_stride)
    h = torch.cuda.current_stream().cuda_stream
    return seg._L.gg_track_clusters(seg._ctx, C.byref(x), C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check(host, want, n, M, order, plane_stride, tag, give_plane=True):
    """a downloaded Dest against tracks_ref.track_maps' answer, every word of it"""
    recs, heads, planes = want
    tracks = host["tracks"]
    for i in range(n):
        Kc = len(recs[i])
        got = tracks[i * M * 8: (i + 1) * M * 8].reshape(M, 8)
        assert heads[i][1] == Kc
        assert np.array_equal(got[:Kc], recs[i].view(np.int32).reshape(Kc, 8)), f"{tag}: map {i}: records"
        assert np.all(got[Kc:] == SIGNED_SENTINEL), f"{tag}: map {i}: a record from Kc on was written"
        assert np.array_equal(host["heads"][4 * i: 4 * i + 4], heads[i]), f"{tag}: map {i}: heads {host['heads'][4 * i: 4 * i + 4]} != {heads[i]}"
        words = host["plane"][i * plane_stride: (i + 1) * plane_stride]
        if give_plane:
            cells = planes[i].size
            assert np.array_equal(words[:cells], planes[i].ravel()), f"{tag}: map {i}: cell_track"
            assert np.all(words[cells:] == SIGNED_SENTINEL), f"{tag}: map {i}: a word beyond rows * cols was written"
    assert np.all(tracks[n * M * 8:] == SIGNED_SENTINEL) and np.all(host["heads"][4 * n:] == SIGNED_SENTINEL)
    assert np.all(host["plane"][n * plane_stride if give_plane else 0:] == SIGNED_SENTINEL)


def stored(planes_rc, order):
    """[n, rows, cols] planes in the shape the call stores them"""
    return np.stack([lay(p, order) for p in planes_rc])


def prior_of(rng, prev_planes, M, wild=False):
    """the record and head buffers a previous call would have left for `prev_planes` (ages and first ids varied)"""
    n = len(prev_planes)
    tracks_in, heads_in = np.zeros((n, M, 8), np.int32), np.zeros((n, 4), np.int32)
    for i, p in enumerate(prev_planes):
        tracks_in[i], heads_in[i] = tracks_ref.first_records(p, M, first_id=int(rng.integers(0, 5000)))
        k = heads_in[i][1]
        tracks_in[i, :k, 1] = rng.integers(0, 50, k)
        if wild and k:
            tracks_in[i, 0, 1] = 2 ** 31 - 1  # an age that saturates
            heads_in[i, 0] = 2 ** 31 - 2      # ids that wrap
    return tracks_in, heads_in


def scene_pair(rng, side, density, shift):
    """(cur, prev) id planes: prev is what cur lies over under `shift`, with 15 % of its cells gone and 3 % added"""
    cur_occ = rng.random((side, side)) < density
    prev_occ = np.roll(cur_occ, (shift[0] % side, shift[1] % side), (0, 1)) if max(abs(shift[0]), abs(shift[1])) < side else rng.random((side, side)) < density
    prev_occ = (prev_occ & (rng.random((side, side)) < 0.85)) | (rng.random((side, side)) < 0.03)
    return tracks_ref.label_plane(cur_occ), tracks_ref.label_plane(prev_occ)


def shifts_of(side):
    return [(0, 0), (1, -2), (side - 1, 0), (-(side - 1), side - 1), (side, 0), (0, -side), (3 * side, 2), (-2, -(side + 5)), (-3, 1), (-side, side)]


def run_and_check(seg, cur, prev, tracks_in, heads_in, shifts, M, g, order, stride, tag, give_plane=True, slack=7):
    import torch

    n, side = len(cur), seg.rows
    dest = Dest(n, M, stride, slack)
    prior = prev is not None
    rc = raw_track(seg, n, dest, pack(cur, order, stride), stride, pack(prev, order, stride + 2) if prior else None, stride + 2 if prior else 0,
                   upload(tracks_in) if prior else None, upload(heads_in) if prior else None, shifts, M, g, order, give_plane)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    want = tracks_ref.track_maps(stored(cur, order), stored(prev, order) if prior else None, tracks_in, heads_in, shifts, M, g, ORDER[order])
    check(dest.host(), want, n, M, order, stride, tag, give_plane)
    return want


# ---------------------------------------------------------------- 1. scenes

@pytest.mark.parametrize("side,density,order,g,n,extra", [
    (23, 0.05, ROW, 0, 1, 0), (23, 0.2, COL, 1, 3, 5), (23, 0.5, ROW, 4, N_SLOTS, 1), (41, 0.05, COL, 4, N_SLOTS, 0),
    (41, 0.2, ROW, 1, N_SLOTS, 3), (41, 0.5, COL, 0, 3, 64), (41, 0.2, COL, 4, 1, 0), (23, 0.2, ROW, 0, N_SLOTS, 0)])
def test_random_scenes(contexts, side, density, order, g, n, extra):
    seg = contexts(side)
    rng = np.random.default_rng(1000 * side + int(100 * density) + 10 * g + n)
    shifts = [shifts_of(side)[(i + g + n) % 4] for i in range(n)]  # (0 and the small ones, side - 1: the rest is test_shifts')
    pairs = [scene_pair(rng, side, density, s) for s in shifts]
    cur, prev = [p[0] for p in pairs], [p[1] for p in pairs]
    tracks_in, heads_in = prior_of(rng, prev, 256, wild=True)
    want = run_and_check(seg, cur, prev, tracks_in, heads_in, shifts, 256, g, order, side * side + extra, f"{side} {density} {order} g{g} n{n}")
    assert sum(int((r["prev"] >= 0).sum()) for r in want[0]) > 0
    run_and_check(seg, cur, prev, tracks_in, heads_in, shifts, 256, g, order, side * side + extra, "no plane", give_plane=False)


@pytest.mark.parametrize("side,order", [(23, ROW), (41, COL)])
def test_shifts(contexts, side, order):
    """0, small, +-(side - 1), +-side and beyond; from |s| = side on everything is born, whatever the gate"""
    seg = contexts(side)
    rng = np.random.default_rng(77 + side)
    every = shifts_of(side)
    for g, part in ((1, every[:5]), (4, every[5:])):
        pairs = [scene_pair(rng, side, 0.2, s) for s in part]
        cur, prev = [p[0] for p in pairs], [p[1] for p in pairs]
        tracks_in, heads_in = prior_of(rng, prev, 256)
        recs, heads, _ = run_and_check(seg, cur, prev, tracks_in, heads_in, part, 256, g, order, side * side + 1, f"shifts g{g}")
        for s, r, h, hin in zip(part, recs, heads, heads_in):
            if abs(s[0]) >= side or abs(s[1]) >= side:
                assert np.all(r["prev"] == -1) and h[2] == len(r) > 0 and h[3] == hin[1]
            elif max(abs(s[0]), abs(s[1])) <= 3:
                assert (r["prev"] >= 0).sum() > 0
    # a NULL shifts is (0, 0)
    cur, prev = scene_pair(rng, side, 0.2, (0, 0))
    tracks_in, heads_in = prior_of(rng, [prev], 256)
    run_and_check(seg, [cur], [prev], tracks_in, heads_in, None, 256, 1, order, side * side, "null shifts")


@pytest.mark.parametrize("side,order", [(23, COL), (41, ROW)])
def test_no_prior(contexts, side, order):
    seg = contexts(side)
    rng = np.random.default_rng(5 + side)
    cur = [tracks_ref.random_scene(rng, side, d) for d in (0.05, 0.2, 0.5)] + [np.full((side, side), -1, np.int32)]
    recs, heads, _ = run_and_check(seg, cur, None, None, None, [(1, 1)] * 4, 256, 1, order, side * side + 2, "no prior")
    for r, h in zip(recs, heads):
        assert r["track_id"].tolist() == list(range(len(r))) and not r["age"].any() and h.tolist() == [len(r), len(r), len(r), 0]
    assert len(recs[3]) == 0 and len(recs[1]) > 10


# ---------------------------------------------------------------- 2. chained frames

def test_three_chained_frames(contexts):
    """the outputs of one call are the prior of the next, as the caller alternates them: ages grow, next_id carries"""
    import torch

    side, M, n, order = 41, 256, 3, ROW
    seg = contexts(side)
    rng = np.random.default_rng(4100)
    stride = side * side
    occ = [rng.random((side, side)) < 0.12 for _ in range(n)]
    frames, shifts = [], [None, [(0, 0), (1, 0), (-1, 2)], [(2, -1), (0, 0), (0, 1)]]
    for f in range(3):
        if f:
            occ = [(np.roll(o, (-s[0], -s[1]), (0, 1)) & (rng.random((side, side)) < 0.9)) | (rng.random((side, side)) < 0.01) for o, s in zip(occ, shifts[f])]
        frames.append([tracks_ref.label_plane(o) for o in occ])
    dests = [Dest(n, M, stride) for _ in range(3)]
    bufs = [pack(fr, order, stride) for fr in frames]
    for f in range(3):
        prior = dict(prev=bufs[f - 1], prev_stride=stride, tracks_in=dests[f - 1].tracks, heads_in=dests[f - 1].heads) if f else {}
        assert raw_track(seg, n, dests[f], bufs[f], stride, shifts=shifts[f], M=M, g=1, order=order, **prior) == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    tracks_in = heads_in = None
    oldest = 0
    for f in range(3):
        want = tracks_ref.track_maps(stored(frames[f], order), stored(frames[f - 1], order) if f else None, tracks_in, heads_in, shifts[f], M, 1, "row")
        check(dests[f].host(), want, n, M, order, stride, f"frame {f}")
        tracks_in = np.zeros((n, M, 8), np.int32)
        for i, r in enumerate(want[0]):
            tracks_in[i, :len(r)] = r.view(np.int32).reshape(-1, 8)
            oldest = max(oldest, int(r["age"].max()))
        if f:
            assert np.all(want[1][:, 0] == heads_in[:, 0] + want[1][:, 2]) and np.all(want[1][:, 2] > 0)
        heads_in = want[1]
    assert oldest == 2


# ---------------------------------------------------------------- 3. the limits of the cluster count

@pytest.mark.parametrize("side,M", [(41, 4), (41, 256), (41, 1024), (23, 4), (23, 256), (23, 1024)])
def test_more_clusters_than_a_slab_and_than_max_clusters(contexts, side, M):
    """isolated cells: 441 clusters on side 41, 144 on side 23, against a previous plane of as many: more rows than one slab of the
    contingency matrix holds, more clusters than M, ids >= M in either plane; heads_in[1] above M, above the plane's count and negative"""
    seg = contexts(side)
    rng = np.random.default_rng(side + M)
    occ = np.zeros((side, side), bool)
    occ[::2, ::2] = True
    other = np.zeros((side, side), bool)
    other[1::2, 1::2] = True
    other[0, 0] = True
    cur, prev = tracks_ref.label_plane(occ), tracks_ref.label_plane(other)
    count = int(cur.max()) + 1
    assert count == ((side + 1) // 2) ** 2 and count in (441, 144)
    if M == 1024 and side == 41:
        assert count * (int(prev.max()) + 1) > 4 * _lib.GG_TRACK_SLAB_WORDS  # several slabs
    tracks_in = np.zeros((N_SLOTS, M, 8), np.int32)
    tracks_in[:, :, 0] = 7000 + 3 * np.arange(M)[None, :] + 10000 * np.arange(N_SLOTS)[:, None]
    tracks_in[:, :, 1] = rng.integers(0, 9, (N_SLOTS, M))
    n_prev = int(prev.max()) + 1
    heads_in = np.array([[50, n_prev, 0, 0], [60, M + 5000, 0, 0], [70, -3, 0, 0], [2 ** 31 - 3, min(n_prev, M) // 2, 0, 0], [-5, 2 ** 31 - 1, 0, 0]], np.int32)
    shifts = [(0, 0), (1, 0), (0, 0), (-1, -1), (0, 1)]
    for g in (1, 4):
        want = run_and_check(seg, [cur] * N_SLOTS, [prev, prev, prev, cur, cur], tracks_in, heads_in, shifts, M, g, ROW, side * side + 3, f"M{M} g{g}")
        assert all(len(r) == min(count, M) for r in want[0]) and want[1][2].tolist() == [70 + min(count, M), min(count, M), min(count, M), 0]


# ---------------------------------------------------------------- 4. splits, merges and ties

@pytest.mark.parametrize("order", [ROW, COL])
def test_splits_merges_and_ties(contexts, order):
    side, M = 23, 8
    seg = contexts(side)

    def plane(*boxes):
        p = np.full((side, side), -1, np.int32)
        for k, (r0, r1, c0, c1) in enumerate(boxes):
            p[r0:r1, c0:c1] = k
        return p

    whole, wide = (5, 7, 2, 12), (15, 17, 2, 12)
    cases = [  # (cur, prev, what the records must say)
        (plane((5, 7, 2, 5), (5, 7, 6, 12)), plane(whole), dict(prev=[-1, 0])),             # a split, unequal: the larger part
        (plane((5, 7, 2, 6), (5, 7, 8, 12)), plane(whole), dict(prev=[0, -1])),             # a split, equal: a tie on c, the smaller c
        (plane(whole), plane((5, 7, 2, 5), (5, 7, 6, 12)), dict(prev=[1])),                 # a merge: the larger overlap
        (plane(whole), plane((5, 7, 2, 6), (5, 7, 8, 12)), dict(prev=[0])),                 # a merge, equal: a tie on p, the smaller p
        (plane((5, 7, 2, 6), (5, 7, 8, 12), wide), plane(whole, (15, 17, 2, 6), (15, 17, 8, 12)), dict(prev=[0, -1, 1])),  # both at once
    ]
    rng = np.random.default_rng(9)
    cur, prev = [c[0] for c in cases], [c[1] for c in cases]
    tracks_in, heads_in = prior_of(rng, prev, M)
    for g in (0, 1):
        recs, heads, _ = run_and_check(seg, cur, prev, tracks_in, heads_in, None, M, g, order, side * side, f"splits g{g}")
        for (_, _, say), r, h, hin in zip(cases, recs, heads, heads_in):
            assert r["prev"].tolist() == say["prev"]
            assert h[3] == hin[1] - sum(p >= 0 for p in say["prev"]) and h[2] == sum(p < 0 for p in say["prev"])


# ---------------------------------------------------------------- 5. twice the same

def test_twice_the_same(contexts):
    import torch

    side, M, n = 41, 1024, N_SLOTS
    seg = contexts(side)
    rng = np.random.default_rng(31)
    pairs = [scene_pair(rng, side, 0.3, (1, -1)) for _ in range(n)]
    cur, prev = [p[0] for p in pairs], [p[1] for p in pairs]
    tracks_in, heads_in = prior_of(rng, prev, M)
    stride = side * side
    d_cur, d_prev, d_tin, d_hin = pack(cur, ROW, stride), pack(prev, ROW, stride), upload(tracks_in), upload(heads_in)
    dests = [Dest(n, M, stride) for _ in range(2)]
    for d in dests:
        assert raw_track(seg, n, d, d_cur, stride, d_prev, stride, d_tin, d_hin, [(1, -1)] * n, M, 2, ROW) == 0
    torch.cuda.synchronize()
    a, b = dests[0].host(), dests[1].host()
    assert all(a[k].tobytes() == b[k].tobytes() for k in Dest.FIELDS) and not dests[0].all_sentinel()


# ---------------------------------------------------------------- 6. errors write nothing

def test_errors_write_nothing(contexts):
    import torch

    side, M, n = 23, 16, 2
    seg = contexts(side)
    cells = side * side
    rng = np.random.default_rng(3)
    cur, prev = scene_pair(rng, side, 0.2, (0, 0))
    tracks_in, heads_in = prior_of(rng, [prev] * n, M)
    d_cur, d_prev, d_tin, d_hin = pack([cur] * n, ROW, cells), pack([prev] * n, ROW, cells), upload(tracks_in), upload(heads_in)
    dest = Dest(n, M, cells)

    def call(status, n_maps=n, cells_buf=d_cur, cells_stride=cells, prior=(d_prev, d_tin, d_hin), prev_stride=cells, **kw):
        args = dict(M=M, g=1, order=ROW)
        args.update(kw)
        rc = raw_track(seg, n_maps, dest, cells_buf, cells_stride, prior[0], prev_stride, prior[1], prior[2], None, **args)
        assert rc == status, (rc, kw, seg._L.gg_last_error(seg._ctx))
        torch.cuda.synchronize()
        assert dest.all_sentinel(), kw

    assert seg._L.gg_track_clusters(seg._ctx, None, None) == INVALID
    call(INVALID, n_maps=-1)
    call(INVALID, cells_buf=None)
    call(INVALID, tracks_out=0)
    call(INVALID, heads_out=0)
    for some in ((d_prev, None, None), (None, d_tin, None), (None, None, d_hin), (d_prev, d_tin, None), (d_prev, None, d_hin), (None, d_tin, d_hin)):
        call(INVALID, prior=some)
    call(INVALID, cells_stride=cells - 1)
    call(INVALID, prev_stride=cells - 1)
    call(INVALID, track_stride=cells - 1)
    call(INVALID, order=2)
    call(INVALID, order=-1)
    for bad in (0, -1, _lib.GG_TRACK_MAX_CLUSTERS + 1):
        call(INVALID, M=bad)
    for bad in (-1, 5):
        call(INVALID, g=bad)
    # an output that overlaps an input or another output
    call(INVALID, cell_track=d_cur)
    call(INVALID, cell_track=d_prev.data_ptr() + 4 * (cells - 1))
    call(INVALID, tracks_out=d_tin)
    call(INVALID, heads_out=d_hin)
    call(INVALID, tracks_out=d_cur)
    call(INVALID, heads_out=dest.tracks.data_ptr() + 4 * (n * M * 8 - 1))
    call(INVALID, cell_track=dest.tracks.data_ptr() + 32 * (n * M - 1), track_stride=cells)
    call(INVALID, heads_out=dest.plane.data_ptr() + 4 * (n * cells - 1))
    call(CAPACITY, n_maps=N_SLOTS + 1)
    # n == 0 is GG_OK before anything else is looked at
    assert raw_track(seg, 0, dest, None, 0, M=0, g=9, order=7, tracks_out=0, heads_out=0) == 0
    # and the inputs may overlap each other: the previous plane is the current one
    assert raw_track(seg, n, dest, d_cur, cells, d_cur, cells, d_tin, d_hin, None, M, 1, ROW) == 0
    torch.cuda.synchronize()
    assert not dest.all_sentinel()


def test_a_map_whose_coordinate_sums_leave_an_int32_is_refused():
    """rows * cols * max(rows, cols) > 2^31 - 1 from a side of 1291 on: GG_ERR_GEOMETRY, nothing written"""
    import torch

    side = 1291
    assert side ** 3 > 2 ** 31 - 1 >= (side - 1) ** 3
    seg = api.GroundSegmentation().init(float(side), 1.0, n_slots=1, max_points=64)
    assert seg.rows == seg.cols == side
    cells = side * side
    d_cur = torch.full((cells,), -1, dtype=torch.int32, device="cuda")
    dest = Dest(1, 4, cells)
    assert raw_track(seg, 1, dest, d_cur, cells, M=4, g=0, order=ROW) == GEOMETRY_ERR
    torch.cuda.synchronize()
    assert dest.all_sentinel()
    seg.close()


# ---------------------------------------------------------------- 7. the Python entry point and the chain on a drive

def test_python_entry_point(contexts):
    import torch

    side, n, M = 41, 3, 64
    seg = contexts(side)
    rng = np.random.default_rng(64)
    for order in ("row", "col"):
        code = ROW if order == "row" else COL
        pairs = [scene_pair(rng, side, 0.15, (1, 2)) for _ in range(n)]
        cur, prev = stored([p[0] for p in pairs], code), stored([p[1] for p in pairs], code)
        first = seg.track_clusters(upload(prev), max_clusters=M, order=order, on_torch_stream=True)
        second = seg.track_clusters(upload(cur), first, [(1, 2)] * n, M, 2, True, order=order, on_torch_stream=True)
        again = seg.track_clusters(second.cell_cluster, first, [(1, 2)] * n, M, 2, True, out=second, order=order, on_torch_stream=True)
        torch.cuda.synchronize()
        assert again is second and first.cell_track is None and second.cell_cluster.shape == (n, side, side)
        w1 = tracks_ref.track_maps(prev, M=M, g=1, order=order)
        tin = np.zeros((n, M, 8), np.int32)
        for i, r in enumerate(w1[0]):
            tin[i, :len(r)] = r.view(np.int32).reshape(-1, 8)
        w2 = tracks_ref.track_maps(cur, prev, tin, w1[1], [(1, 2)] * n, M, 2, order)
        assert np.array_equal(first.heads.cpu().numpy(), w1[1]) and np.array_equal(second.heads.cpu().numpy(), w2[1])
        assert np.array_equal(second.cell_track.cpu().numpy(), w2[2])
        for i in range(n):
            assert second.table(i).tolist() == w2[0][i].tolist() and first.table(i).tolist() == w1[0][i].tolist()
        motion = second.motion(first, [(1, 2)] * n, resolution=0.5)
        kept = w2[0][0]["prev"] >= 0
        assert motion.shape == (n, M, 2) and np.isfinite(motion[0, :len(kept)][kept]).all() and np.isnan(motion[0, :len(kept)][~kept]).all()
        with pytest.raises(ValueError):
            seg.track_clusters(second.cell_cluster, first, out=first, max_clusters=M, order=order)
        with pytest.raises(ValueError):
            seg.track_clusters(second.cell_cluster, first, max_clusters=M + 1, order=order)
        with pytest.raises(ValueError):
            seg.track_clusters(second.cell_cluster, max_clusters=_lib.GG_TRACK_MAX_CLUSTERS + 1, order=order)
        with pytest.raises(ValueError):
            seg.track_clusters(second.cell_cluster, gate=5, order=order)
        with pytest.raises(ValueError):
            seg.track_clusters(second.cell_cluster.to(torch.int64), order=order)


def test_two_frames_of_a_drive():
    """filter_batch -> cluster_clouds -> track_clusters on two synthetic frames with a move_maps between them, against the reference fed
    with the downloaded id planes; the world stands still, so clusters keep their identity"""
    import torch

    K, M = 2, 1024
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=K, max_points=20000)
    seg.reset_maps(odom_z=0.0)
    clouds = [synth.hdl64_cloud(seed=2300 + k, n_az=160 + 20 * k) for k in range(K)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    pts = batch_points(clouds, stride)
    odoms = [np.zeros((K, 2)), np.array([[1.1, -0.8], [-0.5, 0.7]])]
    ids, outs, shifts, prev = [api.ClusterOutputs(), api.ClusterOutputs()], [], None, None
    for f in range(2):
        moved = np.array(seg.move_maps(odoms[f], [POSE] * K, on_torch_stream=True))
        shifts = moved if f else None
        res = seg.filter_batch(pts, n_pts, np.zeros((K, 3), np.float32), np.full(K, -1.73), want_masks=True)
        cl = seg.cluster_clouds(pts, n_pts, masks=res.label_masks, max_clusters=M, point_clusters=False, out=ids[f])
        prev = seg.track_clusters(cl.cell_cluster, prev, shifts, M, 1, True, on_torch_stream=True)
        outs.append(prev)
    torch.cuda.synchronize()
    assert np.abs(shifts).max() >= 2
    planes = [o.cell_cluster.cpu().numpy() for o in outs]
    w1 = tracks_ref.track_maps(planes[0], M=M, g=1)
    tin = np.zeros((K, M, 8), np.int32)
    for i, r in enumerate(w1[0]):
        tin[i, :len(r)] = r.view(np.int32).reshape(-1, 8)
    w2 = tracks_ref.track_maps(planes[1], planes[0], tin, w1[1], shifts, M, 1)
    for o, w in zip(outs, (w1, w2)):
        assert np.array_equal(o.heads.cpu().numpy(), w[1]) and np.array_equal(o.cell_track.cpu().numpy(), w[2])
        for i in range(K):
            assert o.table(i).tolist() == w[0][i].tolist()
    for i in range(K):
        Kc, born, ended = (int(v) for v in w2[1][i][1:])
        print(f"map {i}: shift {shifts[i].tolist()}, {int(w1[1][i][1])} -> {Kc} clusters, born {born}, ended {ended}")
        assert Kc > 20 and Kc - born > 0
    seg.close()
