"""gg_split_clouds (the ground and the non-ground points of many labelled clouds as dense clouds in device memory, with heights above the
terrain and source indices, one call) on the device.  Expected values come from the CPU oracle alone: OracleMap.filter_cloud gives the
labels per input point and the `ground` layer afterwards, OracleMap.get_index the cell, numpy `labels == 49 / 99` the selection and
np.float32(z) - ground[row, col] the height.  Every comparison is on bits, except that a NaN height (a NaN z) is compared as "is NaN"."""
import ctypes as C
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
from tests.cloud_refs import CODE, QUIET_NAN, SETS, expected_sets  # noqa: E402
from tests.test_export_layers_gpu import SENTINEL, batch_points, fresh_count, same_bits, stride_of, warm_maps  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY = -1, -5
FIELDS = ("points", "height", "source")
PARAM_RING = 4  # (gg_context.hip: entries of a call's parameter ring)
GEOMETRY = {79: (26.0, 0.33), 364: (120.0, 0.33)}
SIGNED_SENTINEL = SENTINEL - (1 << 32) if SENTINEL >= (1 << 31) else SENTINEL


# ---------------------------------------------------------------- helpers

def lazy_count(seg):
    """how many maps still owe the three lazily kept layers of their last cloud"""
    return seg.debug_set_tuning("lazy_count", 0)


def points_tensor(clouds, stride, fmt):
    """[B, stride, 16] packed records or [B, stride, 32] PointXYZIR, uint8, on the device"""
    import torch

    if fmt == _lib.GG_POINT16:
        return batch_points(clouds, stride)
    host = np.zeros((len(clouds), stride, 32), dtype=np.uint8)
    for b, c in enumerate(clouds):
        host[b, : len(c)] = np.frombuffer(c.tobytes(), dtype=np.uint8).reshape(-1, 32)
    return torch.from_numpy(host).cuda()


def masks_of(labels, stride):
    """the 2-bit masks of gg_batch.d_label_masks from label bytes [B, stride] (host): 49 -> 1, 99 -> 2, everything else 0"""
    code = np.where(labels == 49, 1, np.where(labels == 99, 2, 0)).astype(np.uint8).reshape(labels.shape[0], stride // 4, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8)


class Outputs:
    """sentinel-filled destinations of one call; want = {set: fields} names the pointers that are handed over"""

    def __init__(self, n, stride, want=None):
        import torch

        self.n, self.stride = n, stride
        self.want = {s: FIELDS for s in SETS} if want is None else want
        words = {"points": 4, "height": 1, "source": 1}
        self.t = {(s, k): torch.full((n * stride * words[k],), SIGNED_SENTINEL, dtype=torch.int32, device="cuda") for s in SETS for k in FIELDS}
        self.counts = torch.full((n * 2,), SIGNED_SENTINEL, dtype=torch.int32, device="cuda")

    def ptr(self, s, k):
        return self.t[(s, k)].data_ptr() if k in self.want.get(s, ()) else 0

    def host(self):
        h = {key: t.cpu().numpy().view(np.uint32) for key, t in self.t.items()}
        return h, self.counts.cpu().numpy().reshape(self.n, 2)


def raw_split(seg, n, slots, first_slot, fmt, points, stride, n_points, out, labels=0, masks=0, transforms=None, counts="out", stream=None, own=False):
    """gg_split_clouds as the C ABI has it (device addresses as integers, 0 = null); returns the status"""
    import torch

    x = _lib.GGCloudSplit()
    sl = None if slots is None else (C.c_int32 * max(len(slots), 1))(*[int(s) for s in slots])
    npts = None if n_points is None else (C.c_int32 * max(len(n_points), 1))(*[int(v) for v in n_points])
    x.n, x.first_slot, x.slots, x.point_format = n, first_slot, sl, fmt
    x.d_points, x.cloud_stride, x.n_points = points or None, stride, npts
    tfs = None
    if transforms is not None:
        tfs = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(-1, 12))
        x.transforms = tfs.ctypes.data_as(C.POINTER(C.c_double))
    x.d_labels, x.d_label_masks = labels or None, masks or None
    for s, dst in (("ground", x.ground), ("nonground", x.nonground)):
        for k in FIELDS:
            setattr(dst, "d_" + k, out.ptr(s, k) or None)
    x.d_counts = (out.counts.data_ptr() if counts == "out" else counts) or None
    h = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return seg._L.gg_split_clouds(seg._ctx, C.byref(x), None if own else C.c_void_p(h if h else _lib.GG_STREAM_DEFAULT))


def check_cloud(host, counts, i, stride, want, tag, given=None):
    """cloud i of a downloaded Outputs against expected_sets; `given` = {set: fields} that were handed over (default: everything)"""
    given = {s: FIELDS for s in SETS} if given is None else given
    for col, s in enumerate(SETS):
        idx, recs, h = want[s]
        m = len(idx)
        assert counts[i, col] == m, f"{tag}: cloud {i} {s}: count {counts[i, col]} against {m}"
        for k in FIELDS:
            words = 4 if k == "points" else 1
            row = host[(s, k)][i * stride * words: (i + 1) * stride * words]
            if k not in given.get(s, ()):
                assert np.all(row == SENTINEL), f"{tag}: cloud {i} {s}.{k} was not asked for and was written"
                continue
            assert np.all(row[m * words:] == SENTINEL), f"{tag}: cloud {i} {s}.{k}: elements at or beyond the count were written"
            got = row[: m * words]
            if k == "points":
                assert got.tobytes() == recs.tobytes(), f"{tag}: cloud {i} {s}: {int((got.reshape(-1, 4) != np.frombuffer(recs.tobytes(), dtype=np.uint32).reshape(-1, 4)).any(axis=1).sum())} records differ"
            elif k == "source":
                assert np.array_equal(got.view(np.int32), idx), f"{tag}: cloud {i} {s}: source"
            else:
                nan = np.isnan(h)
                assert np.array_equal(np.isnan(got.view(np.float32)), nan), f"{tag}: cloud {i} {s}: NaN heights"
                assert np.array_equal(got[~nan], h.view(np.uint32)[~nan]), f"{tag}: cloud {i} {s}: {int((got[~nan] != h.view(np.uint32)[~nan]).sum())} heights differ"


def transform_of():
    q = np.array([0.01, -0.02, np.sin(0.4), np.cos(0.4)])
    q /= np.linalg.norm(q)
    R, t = kitti.matrix_from_quaternion(q), np.array([0.75, -0.5, 0.07])
    return R, t, np.hstack([R, t[:, None]])


def lengths_scene(size, fmt, use_tf, monkeypatch=None):
    """Eleven maps through a non-consecutive slot list -- five warmed by two scrolled batches, six as the reset left them --, then one batch
    of distinct clouds of the lengths full, full (a random cloud whose extent exceeds the map), 4 * 128 + 1, 129, 128, 127, 65, 64, 63, 1, 0.
    Returns the context, the batch's device tensors and per cloud the oracle's expected_sets."""
    import torch

    length, res = GEOMETRY[size]
    if monkeypatch is not None:
        monkeypatch.setenv("GG_PW", "128")  # (read at gg_create: a 1500-point cloud spans 12 chunks and 3 work-groups)
    slots = [11, 2, 7, 0, 9, 4, 12, 1, 6, 10, 3]
    seg = api.GroundSegmentation().init(length, res, n_slots=13, max_points=20000)
    if monkeypatch is not None:
        assert seg.debug_set_tuning("pw", 0) == 128
    assert seg.rows == seg.cols == size
    seg.reset_maps(odom_z=0.2)
    refs = [oracle.OracleMap(length, res, odom_z=0.2) for _ in slots]
    warm_maps(seg, slots[:5], seed=3100, refs=refs[:5])
    extent = 0.6 * length
    clouds = [synth.hdl64_cloud(seed=3150, n_az=150), synth.random_cloud(1500, seed=3151, extent=extent)]
    clouds += [synth.random_cloud(m, seed=3160 + m, extent=extent) for m in (4 * 128 + 1, 129, 128, 127, 65, 64, 63, 1)]
    clouds.append(synth.empty_cloud(0))
    n_pts = [len(c) for c in clouds]
    assert n_pts[2:] == [513, 129, 128, 127, 65, 64, 63, 1, 0] and n_pts[0] > 1500
    stride = stride_of(clouds)
    R, t, tf = transform_of()
    maps = [kitti.transform_cloud(c, R, t) if len(c) else c for c in clouds] if use_tf else clouds  # what the nodelet computes on the CPU (Nodelet.cpp:166-181)
    origin = tuple(np.float32(v) for v in t) if use_tf else (0.0, 0.0, 0.0)
    pts = points_tensor(clouds, stride, fmt)
    out = seg.filter_batch(pts, n_pts, [origin] * len(slots), np.full(len(slots), -1.73), slots=slots, want_masks=True,
                           transforms=[tf] * len(slots) if use_tf else None)
    torch.cuda.synchronize()
    labels = out.labels.cpu().numpy()
    want = []
    for i in range(len(slots)):
        r = refs[i].filter_cloud(maps[i], origin, -1.73)
        assert np.array_equal(labels[i, : n_pts[i]], r["label"]), f"cloud {i}: the batch's labels are not the oracle's"
        want.append(expected_sets(refs[i], maps[i], r["label"]))
    # The 2-bit masks of the same labels.  k_label's windows come four at a time and every window writes its mask bytes, so with chunks of
    # fewer than 256 points (GG_PW=128, a tests-only setting) a chunk's last iteration writes zero codes over the bytes of the chunk behind
    # it: there the masks are packed on the host from the labels that were just held to the oracle's; with the library's own chunk sizes
    # (multiples of 256) the batch's masks are handed over as they are, after the same packing has been held against them
    host_masks = masks_of(np.where(np.arange(stride)[None, :] < np.array(n_pts)[:, None], labels, 0).astype(np.uint8), stride)
    if monkeypatch is None:
        got_masks = out.label_masks.cpu().numpy()
        for i in range(len(slots)):
            assert np.array_equal(got_masks[i, : (n_pts[i] + 3) // 4], host_masks[i, : (n_pts[i] + 3) // 4]), f"cloud {i}: the batch's masks are not its labels"
        masks = out.label_masks
    else:
        masks = torch.from_numpy(host_masks).cuda()
    assert sum(len(w["ground"][0]) for w in want) > 500 and sum(len(w["nonground"][0]) for w in want) > 500
    dropped = n_pts[1] - len(want[1]["ground"][0]) - len(want[1]["nonground"][0])
    assert dropped > 50, "the random cloud has too few dropped points between the selected ones"
    return dict(seg=seg, slots=slots, pts=pts, n_pts=n_pts, stride=stride, out=out, masks=masks, want=want, tf=[tf] * len(slots) if use_tf else None, fmt=fmt)


# ---------------------------------------------------------------- 1. parity with the oracle

@pytest.mark.parametrize("use_tf", [False, True])
@pytest.mark.parametrize("use_masks", [False, True])
@pytest.mark.parametrize("fmt", [_lib.GG_POINT16, _lib.GG_POINT32])
@pytest.mark.parametrize("size,small_chunks", [(79, True), (364, False)])
def test_parity_with_the_oracle(size, small_chunks, fmt, use_masks, use_tf, monkeypatch):
    import torch

    sc = lengths_scene(size, fmt, use_tf, monkeypatch if small_chunks else None)
    seg, n = sc["seg"], len(sc["slots"])
    fresh_before = fresh_count(seg)
    o = Outputs(n, sc["stride"])
    lab = dict(masks=sc["masks"].data_ptr()) if use_masks else dict(labels=sc["out"].labels.data_ptr())
    rc = raw_split(seg, n, sc["slots"], 0, fmt, sc["pts"].data_ptr(), sc["stride"], sc["n_pts"], o, transforms=sc["tf"], **lab)
    assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    assert fresh_count(seg) == fresh_before
    host, counts = o.host()
    tag = f"{size} {'point16' if fmt else 'point32'} {'masks' if use_masks else 'labels'} {'tf' if use_tf else 'map frame'}"
    for i in range(n):
        check_cloud(host, counts, i, sc["stride"], sc["want"][i], tag)
    seg.close()


# ---------------------------------------------------------------- 2. agreement with the batch's returned cloud

def test_agreement_with_the_returned_cloud():
    import torch

    slots = [3, 0, 2]
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=20000)
    seg.reset_maps(odom_z=0.1)
    warm_maps(seg, slots, seed=3200)
    clouds = [synth.hdl64_cloud(seed=3250 + k, n_az=140 + 11 * k) for k in range(3)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    R, t, tf = transform_of()
    pts = points_tensor(clouds, stride, _lib.GG_POINT32)
    out = seg.filter_batch(pts, n_pts, [tuple(np.float32(v) for v in t)] * 3, np.full(3, -1.73), slots=slots, want_clouds=True, transforms=[tf] * 3)
    res = seg.split_clouds(pts, n_pts, labels=out.labels, transforms=[tf] * 3, slots=slots)
    torch.cuda.synchronize()
    counts, batch_counts = res.counts.cpu().numpy(), out.counts.cpu().numpy()
    returned = out.out_clouds.cpu().numpy().view(synth.POINT_DTYPE).reshape(3, stride)
    index = out.out_index.cpu().numpy()
    for i in range(3):
        assert counts[i, 0] + counts[i, 1] == batch_counts[i, 0], i
        assert counts[i, 0] > 100 and counts[i, 1] > 100
        for col, s in enumerate(SETS):
            m = counts[i, col]
            recs = getattr(res, s + "_points")[i, :m].cpu().numpy().view(api.POINT16_DTYPE).reshape(m)
            src = getattr(res, s + "_source")[i, :m].cpu().numpy()
            ret = returned[i][index[i][src]]
            assert np.all(index[i][src] >= 0)
            assert np.all(ret["intensity"] == np.float32(CODE[s]))
            for k in ("x", "y", "z"):
                assert np.array_equal(recs[k].view(np.uint32), ret[k].view(np.uint32)), (i, s, k)
            assert np.array_equal(recs["ring"], ret["ring"]) and not recs["pad"].any(), (i, s)
    seg.close()


# ---------------------------------------------------------------- 3. what is not written

def test_what_is_not_written():
    import torch

    sc = lengths_scene(79, _lib.GG_POINT16, False)
    seg, n, stride = sc["seg"], len(sc["slots"]), sc["stride"]
    combos = [{"ground": ("source",), "nonground": ("source",)}, {"ground": ("height",), "nonground": ("height",)}, {},
              {"nonground": ("points",)}, {"ground": FIELDS}, {"ground": ("points", "source"), "nonground": ("height",)}]
    outs = [Outputs(n, stride, want) for want in combos]
    for o in outs:
        rc = raw_split(seg, n, sc["slots"], 0, sc["fmt"], sc["pts"].data_ptr(), stride, sc["n_pts"], o, labels=sc["out"].labels.data_ptr())
        assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    for o, want in zip(outs, combos):
        host, counts = o.host()
        for i in range(n):
            check_cloud(host, counts, i, stride, sc["want"][i], f"pointers {want}", given=want)
    seg.close()


# ---------------------------------------------------------------- 4. fresh maps and foreign labels

def test_fresh_maps_and_foreign_labels():
    import torch

    length, res = GEOMETRY[79]
    seg = api.GroundSegmentation().init(length, res, n_slots=3, max_points=20000)
    seg.reset_maps(odom_z=1.25, on_torch_stream=True)
    assert fresh_count(seg) == 3
    clouds = [synth.random_cloud(1500, seed=3400 + k, extent=0.8 * length) for k in range(2)]
    stride, n_pts = stride_of(clouds), [1500, 1500]
    labels = np.zeros((2, stride), dtype=np.uint8)
    labels[:, :] = np.tile(np.array([49, 99, 0, 7], dtype=np.uint8), stride // 4)
    d_labels, d_masks = torch.from_numpy(labels).cuda(), torch.from_numpy(masks_of(labels, stride)).cuda()
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    fresh_ref = oracle.OracleMap(length, res, odom_z=1.25)
    slots = [2, 0]
    outs = [Outputs(2, stride), Outputs(2, stride)]
    assert raw_split(seg, 2, slots, 0, _lib.GG_POINT16, pts.data_ptr(), stride, n_pts, outs[0], labels=d_labels.data_ptr()) == 0
    assert raw_split(seg, 2, slots, 0, _lib.GG_POINT16, pts.data_ptr(), stride, n_pts, outs[1], masks=d_masks.data_ptr()) == 0
    torch.cuda.synchronize()
    assert fresh_count(seg) == 3
    for o, kind in zip(outs, ("labels", "masks")):
        host, counts = o.host()
        for i in range(2):
            want = expected_sets(fresh_ref, clouds[i], labels[i], ground=1.25)
            assert len(want["ground"][0]) == len(want["nonground"][0]) == 375  # (0 and 7 select nothing)
            outside = int(np.isnan(want["ground"][2]).sum() + np.isnan(want["nonground"][2]).sum())
            assert 50 < outside < 700
            hb = host[("ground", "height")][i * stride: i * stride + 375]
            assert np.all(hb[np.isnan(want["ground"][2])] == QUIET_NAN)
            inside = ~np.isnan(want["ground"][2])
            assert np.array_equal(hb[inside], (clouds[i]["z"][want["ground"][0]][inside] - np.float32(1.25)).view(np.uint32))
            check_cloud(host, counts, i, stride, want, f"fresh map, {kind}")
    # the same labels on warm maps read those maps' ground
    refs = [oracle.OracleMap(length, res, odom_z=1.25) for _ in slots]
    warm_maps(seg, slots, seed=3450, refs=refs)
    assert fresh_count(seg) == 1
    o = Outputs(2, stride)
    assert raw_split(seg, 2, slots, 0, _lib.GG_POINT16, pts.data_ptr(), stride, n_pts, o, labels=d_labels.data_ptr()) == 0
    torch.cuda.synchronize()
    assert fresh_count(seg) == 1
    host, counts = o.host()
    for i in range(2):
        want = expected_sets(refs[i], clouds[i], labels[i])
        check_cloud(host, counts, i, stride, want, "warm map, foreign labels")
        assert not same_bits(want["ground"][2], expected_sets(fresh_ref, clouds[i], labels[i], ground=1.25)["ground"][2])
    seg.close()


# ---------------------------------------------------------------- 5. nothing changes

def test_nothing_changes():
    import torch

    slots = [4, 1, 5, 2]
    K = len(slots)
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=20000) for _ in range(2)]
    base = [synth.hdl64_cloud(seed=3500 + k, n_az=150 + 7 * k) for k in range(K)]
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
        if which == 0:  # the split between the two batches, on every map of the context (two of them fresh)
            everything = list(range(6))
            all_pts = torch.zeros((6, stride, 16), dtype=torch.uint8, device="cuda")
            all_labels = torch.full((6, stride), 99, dtype=torch.uint8, device="cuda")
            seg.split_clouds(all_pts, [stride] * 6, labels=all_labels, slots=everything)
            seg.split_clouds(pts[0], n_pts[0], masks=first.label_masks, slots=slots, heights=False)
        # the lazily kept layers are still pending behind the split: their first reader computes them, to the values of the twin
        assert lazy_count(seg) == K
        pending = seg.export_layers(lazy, slots=slots)
        assert lazy_count(seg) == 0
        second = seg.filter_batch(pts[1], n_pts[1], origins, base_z, slots=slots)
        planes = seg.export_layers()
        torch.cuda.synchronize()
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


# ---------------------------------------------------------------- 6. a caller's stream, past the ring, no host synchronisation

@pytest.mark.parametrize("halves", [False, True])
def test_on_a_caller_stream_past_the_ring(halves):
    import torch

    n_slots, slots = 4, [2, 1, 3, 0]  # both halves (boundary 2)
    K, rounds = len(slots), PARAM_RING + 2
    base = [synth.hdl64_cloud(seed=3600 + k, n_az=60 + 5 * k) for k in range(K)]
    stride = stride_of(base)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride)
    if halves:
        seg.set_flags(concurrent_halves=True)
        seg.debug_set_tuning("halves_min_clouds", 2)
    sets = [base, base[::-1]]
    pts = [batch_points(c, stride) for c in sets]
    n_pts = [[len(c) for c in cs] for cs in sets]
    origins, base_z = np.zeros((K, 3), np.float32), np.full(K, -1.73)
    outs = [Outputs(K, stride) for _ in range(rounds)]
    torch.cuda.synchronize()  # (the uploads and the fills ran on torch's default stream)
    stream = torch.cuda.Stream()
    batches = []
    with torch.cuda.stream(stream):
        seg.reset_maps(odom_z=0.0, on_torch_stream=True)
        for r in range(rounds):  # no synchronisation anywhere: every batch has its own label tensor, every split its own outputs
            batches.append(seg.filter_batch(pts[r % 2], n_pts[r % 2], origins, base_z, slots=slots))
            rc = raw_split(seg, K, slots, 0, _lib.GG_POINT16, pts[r % 2].data_ptr(), stride, n_pts[r % 2], outs[r], labels=batches[r].labels.data_ptr())
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
    torch.cuda.synchronize()
    refs = [oracle.OracleMap(120.0, 0.33) for _ in slots]
    for r in range(rounds):
        host, counts = outs[r].host()
        for i in range(K):
            cloud = sets[r % 2][i]
            lab = refs[i].filter_cloud(cloud, (0.0, 0.0, 0.0), -1.73)["label"]
            check_cloud(host, counts, i, stride, expected_sets(refs[i], cloud, lab), f"round {r}, halves {halves}")
    seg.close()


# ---------------------------------------------------------------- 7. errors change nothing

def test_errors_change_nothing():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=4096)
    seg.reset_maps(odom_z=0.4)
    clouds = [synth.hdl64_cloud(seed=3700 + k, n_az=40) for k in range(2)]
    stride, n_pts = stride_of(clouds), [len(c) for c in clouds]
    assert stride <= 4096
    warm_maps(seg, [4, 1], seed=3710, frames=1, n_az=40)
    before = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    fresh_before = fresh_count(seg)
    assert fresh_before == 4
    pts = points_tensor(clouds, stride, _lib.GG_POINT16)
    labels = torch.full((2, stride), 99, dtype=torch.uint8, device="cuda")
    o = Outputs(2, stride)
    P, Lb = pts.data_ptr(), labels.data_ptr()

    def call(n=2, slots=None, first=0, fmt=_lib.GG_POINT16, points=P, stride=stride, n_points=n_pts, labels=Lb, masks=0, counts="out"):
        return raw_split(seg, n, slots, first, fmt, points, stride, n_points, o, labels=labels, masks=masks, counts=counts)

    x = _lib.GGCloudSplit()
    x.n = 2
    assert seg._L.gg_split_clouds(None, C.byref(x), None) == INVALID
    assert seg._L.gg_split_clouds(seg._ctx, None, None) == INVALID
    assert call(n=-1) == INVALID
    assert call(slots=[1, 1]) == INVALID
    assert call(points=0) == INVALID
    assert call(n_points=None) == INVALID
    assert call(counts=0) == INVALID
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
    assert call(n=0, points=0, n_points=None, labels=0, counts=0, fmt=9, stride=10 ** 9) == 0  # n == 0: nothing to do, nothing to check
    torch.cuda.synchronize()
    host, counts = o.host()
    assert all(np.all(v == SENTINEL) for v in host.values()) and np.all(counts.view(np.uint32) == SENTINEL)
    assert fresh_count(seg) == fresh_before
    after = seg.export_layers(["ground", "groundpatch"])
    torch.cuda.synchronize()
    assert same_bits(before.cpu().numpy(), after.cpu().numpy())
    assert call(slots=[4, 1]) == 0, seg._L.gg_last_error(seg._ctx)  # ... and the same arguments without a mistake are accepted
    torch.cuda.synchronize()
    host, counts = o.host()
    assert counts.tolist() == [[0, n_pts[0]], [0, n_pts[1]]] and fresh_count(seg) == fresh_before
    assert np.array_equal(host[("nonground", "source")][:n_pts[0]], np.arange(n_pts[0], dtype=np.uint32))
    seg.close()


# ---------------------------------------------------------------- 8. the Python entry point

def test_python_entry_point():
    import torch

    sc = lengths_scene(79, _lib.GG_POINT16, False)
    seg, n, stride, slots = sc["seg"], len(sc["slots"]), sc["stride"], sc["slots"]
    a = seg.split_clouds(sc["pts"], sc["n_pts"], labels=sc["out"].labels, slots=slots)
    assert a.counts.shape == (n, 2) and a.counts.dtype == torch.int32 and a.counts.is_cuda
    for s in SETS:
        p, h, src = (getattr(a, f"{s}_{k}") for k in FIELDS)
        assert p.shape == (n, stride, 16) and p.dtype == torch.uint8 and p.is_cuda
        assert h.shape == (n, stride) and h.dtype == torch.float32
        assert src.shape == (n, stride) and src.dtype == torch.int32
    b = seg.split_clouds(sc["pts"], sc["n_pts"], masks=sc["out"].label_masks, slots=slots, ground=False, heights=False)
    assert b.ground_points is None and b.ground_source is None and b.nonground_height is None and b.nonground_points is not None
    again = seg.split_clouds(sc["pts"], sc["n_pts"], masks=sc["out"].label_masks, slots=slots, ground=False, heights=False, out=b)
    assert again is b
    own = seg.split_clouds(sc["pts"], sc["n_pts"], labels=sc["out"].labels, slots=slots, sources=False, on_torch_stream=False)
    with pytest.raises(ValueError):
        seg.split_clouds(sc["pts"], sc["n_pts"], slots=slots)
    with pytest.raises(ValueError):
        seg.split_clouds(sc["pts"], sc["n_pts"], labels=sc["out"].labels, masks=sc["out"].label_masks, slots=slots)
    with pytest.raises(ValueError):
        seg.split_clouds(sc["pts"], sc["n_pts"], labels=sc["out"].labels, slots=slots, ground=False, heights=False, out=a)  # (tensors that are not asked for)
    torch.cuda.synchronize()
    for res, which in ((a, SETS), (b, ("nonground",)), (own, SETS)):
        for s in which:
            views = res.clouds(s)
            assert len(views) == n
            for i, (p, h, src) in enumerate(views):
                idx, recs, hs = sc["want"][i][s]
                assert p.shape == (len(idx), 16) and p.cpu().numpy().tobytes() == recs.tobytes(), (s, i)
                if src is not None:
                    assert np.array_equal(src.cpu().numpy(), idx), (s, i)
                if h is not None:
                    assert h.shape == (len(idx),) and same_bits(h.cpu().numpy(), hs), (s, i)
    assert own.ground_source is None and b.clouds("nonground")[0][1] is None
    seg.close()
