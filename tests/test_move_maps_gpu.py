"""gg_move_maps (GroundGrid::update for many maps in one set of launches) on the device: bit for bit what one gg_move_map per map gives,
and what the CPU oracle gives, with fresh maps, lazily kept layers, caller streams and GG_FLAG_CONCURRENT_HALVES."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import api, synth  # noqa: E402
from oracle import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

# (odometry offset from the map position, base_to_map pose): the cases of test_map_scroll_edge_cases
CASES = [((0.1, -0.1), (0, 0, 1, 0, 0, 0, 1)),                            # less than half a cell: no move at all
         ((0.17, 0.0), (0.3, 0.2, 1.5, 0.02, -0.01, 0.3, 0.95)),          # just past the rounding point, tilted base
         ((-3.0, 5.2), (1, 2, 3, 0, 0, 0.7071, 0.7071)),                  # negative rows, positive columns
         ((-0.2, -0.7), (0, 0, 0.5, 0.01, 0.02, -0.1, 0.99)),             # negative both ways
         ((40.0, 5.2), (0, 0, 0.5, 0, 0, 0, 1)),                          # more than the whole map in x: everything is new
         ((1e3, -1e3), (0, 0, 0.5, 0.1, 0.2, 0.3, 0.9))]                  # far beyond the map both ways


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def lib_pos(seg, slot):
    """the position the library holds (GridMap.getPosition is the binding's cached copy)"""
    x, y = C.c_double(), C.c_double()
    assert seg._L.gg_get_map_position(seg._ctx, slot, C.byref(x), C.byref(y)) == 0
    return x.value, y.value


def assert_layers_equal(got, want, tag):
    for name in got:
        assert same_bits(got[name], want[name]), f"{tag}: layer {name} differs"


def assert_same_as_oracle(seg_map, ref, tag, names=tuple(oracle.LAYERS)):
    got = seg_map.layers()
    for name in names:
        a, b = got[name], ref.layer(name)
        assert np.array_equal(a, b, equal_nan=True), f"{tag}: layer {name}, {int((a != b).sum())} cells differ"


def batch_points(clouds, stride, fmt=16):
    import torch

    B = len(clouds)
    if fmt == 16:
        host = np.zeros((B, stride), dtype=api.POINT16_DTYPE)
        for b, c in enumerate(clouds):
            host[b, : len(c)] = api.pack16(c)
        raw = host.view(np.uint8).reshape(B, stride, 16)
    else:
        raw = np.zeros((B, stride, 32), dtype=np.uint8)
        for b, c in enumerate(clouds):
            raw[b, : len(c)] = np.frombuffer(c.tobytes(), dtype=np.uint8).reshape(-1, 32)
    return torch.from_numpy(raw).cuda()


def two_contexts(length, res, n_slots, seed, max_points=16):
    """Two contexts with the same random ground / groundpatch and the same (different per slot) positions."""
    segs = [api.GroundSegmentation().init(length, res, n_slots=n_slots, max_points=max_points) for _ in range(2)]
    rng = np.random.default_rng(seed)
    n = segs[0].rows
    init = {}
    for s in range(n_slots):
        g = rng.normal(size=(n, n)).astype(np.float32)
        w = rng.random((n, n)).astype(np.float32)
        pos = (float(rng.integers(-50, 50)) * 0.37, float(rng.integers(-50, 50)) * 0.29)
        init[s] = (g, w, pos)
        for seg in segs:
            seg.map(s).set("ground", g)
            seg.map(s).set("groundpatch", w)
            seg.map(s).setPosition(*pos)
    return segs, init


def moves_for(init, slots, k0=0):
    odoms, poses = [], []
    for k, s in enumerate(slots):
        (dx, dy), pose = CASES[(k + k0) % len(CASES)]
        pos = init[s][2]
        odoms.append((pos[0] + dx, pos[1] + dy))
        poses.append(pose)
    return np.array(odoms), np.array(poses, dtype=np.float64)


@pytest.mark.parametrize("length,res,n_slots,n_moved,chunk", [(120.0, 0.33, 112, 100, 32), (120.0, 0.33, 112, 100, 0), (200.0, 0.2, 7, 6, 2)])
def test_parity_with_the_single_map_call(length, res, n_slots, n_moved, chunk):
    (a, b), init = two_contexts(length, res, n_slots, seed=11)
    if chunk:
        assert a.debug_set_tuning("move_chunk", chunk) == 0
    rng = np.random.default_rng(5)
    slots = [int(s) for s in rng.permutation(n_slots)[:n_moved]]
    odoms, poses = moves_for(init, slots)
    shifts = a.move_maps(odoms, poses, slots=slots)
    for k, s in enumerate(slots):
        want = b.map(s).move(odoms[k][0], odoms[k][1], tuple(poses[k]))
        assert tuple(shifts[k]) == tuple(want), (k, s)
        assert a.map(s).getPosition() == b.map(s).getPosition() == lib_pos(a, s), (k, s)
    assert any(tuple(v) == (0, 0) for v in shifts) and any(abs(v[0]) >= a.rows for v in shifts)
    for s in range(n_slots):
        got = a.map(s).layers(["ground", "groundpatch"])
        assert_layers_equal(got, b.map(s).layers(["ground", "groundpatch"]), f"slot {s}")
        if s not in slots:  # outside the call: untouched
            assert same_bits(got["ground"], init[s][0]) and same_bits(got["groundpatch"], init[s][1]), s
    a.close()
    b.close()


def test_against_the_oracle():
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=16)
    rng = np.random.default_rng(21)
    refs = {}
    slots = [3, 0, 2]
    for s in slots:
        refs[s] = oracle.OracleMap(120.0, 0.33)
        g = rng.normal(size=(seg.rows, seg.cols)).astype(np.float32)
        w = rng.random((seg.rows, seg.cols)).astype(np.float32)
        refs[s].set_layer("ground", g)
        refs[s].set_layer("groundpatch", w)
        seg.map(s).set("ground", g)
        seg.map(s).set("groundpatch", w)
    for step in range(4):
        odoms, poses = [], []
        for k, s in enumerate(slots):
            (dx, dy), pose = CASES[(k + 2 * step) % len(CASES)]
            pos = refs[s].position
            odoms.append((pos[0] + dx, pos[1] + dy))
            poses.append(pose)
        shifts = seg.move_maps(odoms, poses, slots=slots)
        for k, s in enumerate(slots):
            _, want = refs[s].update(odoms[k][0], odoms[k][1], poses[k])
            assert tuple(shifts[k]) == tuple(want), (step, s)
            assert seg.map(s).getPosition() == refs[s].position, (step, s)
            # (the scroll moves the two layers that persist from cloud to cloud, as gg_move_map does: the nine per-call layers are
            # rewritten by the next cloud before anyone can read them -- the filter tests below compare all eleven)
            assert_same_as_oracle(seg.map(s), refs[s], f"step {step} slot {s}", ("ground", "groundpatch"))
    seg.close()


def test_lazily_kept_layers_of_an_earlier_batch():
    import torch

    clouds = [synth.hdl64_cloud(seed=40 + k, n_az=200 + 17 * k) for k in range(4)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=stride) for _ in range(2)]
    pts = batch_points(clouds, stride)
    slots = [4, 1, 5, 2]
    origins = np.zeros((4, 3), np.float32)
    for seg in segs:
        seg.filter_batch(pts, [len(c) for c in clouds], origins, np.full(4, -1.73), slots=slots)
    torch.cuda.synchronize()
    odoms = np.array([(0.8, 0.0), (0.0, -2.5), (0.05, 0.05), (-7.0, 3.1)])
    poses = np.array([CASES[1][1], CASES[2][1], CASES[0][1], CASES[3][1]], dtype=np.float64)
    shifts = segs[0].move_maps(odoms, poses, slots=slots)
    for k, s in enumerate(slots):
        assert tuple(shifts[k]) == tuple(segs[1].map(s).move(odoms[k][0], odoms[k][1], tuple(poses[k])))
    for s in range(6):
        # the layers kept lazily, first through the single-layer getter (the first reader computes them), then all eleven at once
        single = {name: segs[0].map(s)[name] for name in ("maxGroundHeight", "groundCandidates", "planeDist")}
        want = segs[1].map(s).layers()
        assert_layers_equal(single, want, f"slot {s} (single getter)")
        assert_layers_equal(segs[0].map(s).layers(), want, f"slot {s}")
    for seg in segs:
        seg.close()


def test_fresh_maps_moved_then_filtered():
    import torch

    B = 100
    clouds = [synth.hdl64_cloud(seed=700 + k, n_az=96 + (k % 5) * 3) for k in range(B)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    pos0, z0 = (1.3, -0.4), 0.25
    seg.reset_maps(0, B, odom_z=z0, pos=pos0, on_torch_stream=True)
    refs = [oracle.OracleMap(120.0, 0.33, pos=pos0, odom_z=z0) for _ in range(B)]
    rng = np.random.default_rng(8)
    perm = [int(s) for s in rng.permutation(B)]
    moved = perm[:48]  # (CASES[0] is a zero shift: those maps are in the call and stay fresh)
    odoms = np.array([(pos0[0] + CASES[k % len(CASES)][0][0], pos0[1] + CASES[k % len(CASES)][0][1]) for k in range(len(moved))])
    poses = np.array([CASES[k % len(CASES)][1] for k in range(len(moved))], dtype=np.float64)
    shifts = seg.move_maps(odoms, poses, slots=moved, on_torch_stream=True)
    for k, s in enumerate(moved):
        _, want = refs[s].update(odoms[k][0], odoms[k][1], poses[k])
        assert tuple(shifts[k]) == tuple(want)
    still_fresh = [s for k, s in enumerate(moved) if tuple(shifts[k]) == (0, 0)] + perm[48:]
    pts_all = batch_points(clouds, stride, fmt=32)
    origins = np.array([[0.05 * (b % 7), -0.03 * (b % 5), 0.01 * (b % 3)] for b in range(B)], dtype=np.float32)
    base_z = np.array([-1.73 + 0.003 * (b % 9) for b in range(B)])
    # first the maps that are still fresh (a launch that may take them as they are), then every map (moved and filtered ones mixed)
    for tag, order in (("unmoved", still_fresh), ("all", perm)):
        sel = [int(s) for s in order]
        sub = [clouds[s] for s in sel]
        pts = pts_all[sel].contiguous()
        out = seg.filter_batch(pts, [len(c) for c in sub], origins[sel], base_z[sel], slots=sel, want_clouds=True)
        torch.cuda.synchronize()
        labels, counts = out.labels.cpu().numpy(), out.counts.cpu().numpy()
        for b, s in enumerate(sel):
            r = refs[s].filter_cloud(clouds[s], tuple(origins[s]), float(base_z[s]))
            n = len(clouds[s])
            assert np.array_equal(labels[b, :n], r["label"]), (tag, s)
            assert counts[b, 0] == len(r["out_points"]), (tag, s)
            assert out.out_clouds[b, : counts[b, 0]].cpu().numpy().tobytes() == r["out_points"].tobytes(), (tag, s)
    for s in sorted(set(moved[:12]) | set(perm[48:54])):
        assert_same_as_oracle(seg.map(s), refs[s], f"slot {s}")
    seg.close()


def _drive(K, frames):
    """K vehicles: distinct start points and headings, 0.8 m per frame; vehicle 0 stands still, vehicle 1 turns."""
    paths = []
    for v in range(K):
        x, y, th = -20.0 + 5.3 * v, 11.0 - 3.7 * v, 0.7 * v
        speed = 0.0 if v == 0 else 0.8
        turn = 0.12 if v == 1 else 0.0
        p = []
        for f in range(frames):
            p.append((x, y, th))
            th += turn
            x += speed * math.cos(th)
            y += speed * math.sin(th)
        paths.append(p)
    return paths


def _pose(x, y, th):
    """lookupTransform("base_link", "map") of a vehicle at (x, y) with heading th, base 1.73 m above the map plane"""
    c, s = math.cos(-th), math.sin(-th)
    return (-(c * x - s * y), -(s * x + c * y), 1.73, 0.0, 0.0, math.sin(-th / 2), math.cos(-th / 2))


def test_fleet_drive():
    import torch

    K, frames = 8, 20
    paths = _drive(K, frames)
    slots = [6, 2, 9, 0, 4, 7, 1, 3]
    n_slots = 11
    base = [synth.hdl64_cloud(seed=900 + v, n_az=110) for v in range(K)]
    stride = (max(len(c) for c in base) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride)
    refs = [oracle.OracleMap(120.0, 0.33) for _ in range(K)]
    stream = torch.cuda.Stream()
    out = None
    with torch.cuda.stream(stream):
        for f in range(frames):
            odoms = np.array([(paths[v][f][0], paths[v][f][1]) for v in range(K)])
            poses = np.array([_pose(*paths[v][f]) for v in range(K)], dtype=np.float64)
            clouds = []
            for v in range(K):
                c = synth.clone_cloud(base[(v + f) % K])
                c["x"] += np.float32(paths[v][f][0])
                c["y"] += np.float32(paths[v][f][1])
                clouds.append(c)
            origins = np.array([(paths[v][f][0], paths[v][f][1], 0.0) for v in range(K)], dtype=np.float32)
            shifts = seg.move_maps(odoms, poses, slots=slots, on_torch_stream=True)
            out = seg.filter_batch(batch_points(clouds, stride), [len(c) for c in clouds], origins, np.full(K, -1.73), slots=slots, out=out)
            stream.synchronize()
            labels = out.labels.cpu().numpy()
            for v in range(K):
                _, want = refs[v].update(odoms[v][0], odoms[v][1], poses[v])
                assert tuple(shifts[v]) == tuple(want), (f, v)
                r = refs[v].filter_cloud(clouds[v], tuple(origins[v]), -1.73)
                assert np.array_equal(labels[v, : len(clouds[v])], r["label"]), (f, v)
    for v in range(K):
        assert seg.map(slots[v]).getPosition() == refs[v].position
        assert_same_as_oracle(seg.map(slots[v]), refs[v], f"vehicle {v}")
    seg.close()


def test_caller_stream_right_after_a_batch_on_another_stream():
    import torch

    clouds = [synth.hdl64_cloud(seed=60 + k, n_az=300) for k in range(3)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=5, max_points=stride) for _ in range(2)]
    pts = batch_points(clouds, stride)
    torch.cuda.synchronize()  # (the upload ran on torch's default stream, the batch runs on s1)
    slots = [3, 0, 4]
    odoms = np.array([(1.9, -0.6), (-4.0, 0.0), (0.5, 2.2)])
    poses = np.array([CASES[1][1], CASES[2][1], CASES[3][1]], dtype=np.float64)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        segs[0].filter_batch(pts, [len(c) for c in clouds], np.zeros((3, 3), np.float32), np.full(3, -1.73), slots=slots)
    segs[0].move_maps(odoms, poses, slots=slots, stream=s2.cuda_stream)  # no synchronisation in between: the library orders it
    got = {s: segs[0].map(s).layers() for s in range(5)}
    segs[1].filter_batch(pts, [len(c) for c in clouds], np.zeros((3, 3), np.float32), np.full(3, -1.73), slots=slots)
    torch.cuda.synchronize()
    for k, s in enumerate(slots):
        segs[1].map(s).move(odoms[k][0], odoms[k][1], tuple(poses[k]))
    for s in range(5):
        assert_layers_equal(got[s], segs[1].map(s).layers(), f"slot {s}")
    for seg in segs:
        seg.close()


def test_concurrent_halves_alternating_move_and_filter():
    import torch

    n_slots, slots = 16, [2, 9, 5, 12, 7, 8, 15, 0]  # both halves (boundary 8)
    K = len(slots)
    base = [synth.hdl64_cloud(seed=300 + k, n_az=140) for k in range(K)]
    stride = (max(len(c) for c in base) + 63) // 64 * 64
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride) for _ in range(2)]
    segs[0].set_flags(concurrent_halves=True)
    segs[0].debug_set_tuning("halves_min_clouds", 2)
    segs[0].debug_set_tuning("move_chunk", 3)
    stream = torch.cuda.Stream()  # (not the legacy default stream: the halves are not used there)
    outs = [None, None]
    for step in range(4):
        odoms = np.array([(0.8 * step * math.cos(0.3 * k), 0.8 * step * math.sin(0.3 * k) - 0.4 * (k % 2)) for k in range(K)])
        poses = np.array([CASES[(k + step) % len(CASES)][1] for k in range(K)], dtype=np.float64)
        clouds = []
        for k in range(K):
            c = synth.clone_cloud(base[(k + step) % K])
            c["x"] += np.float32(odoms[k][0])
            c["y"] += np.float32(odoms[k][1])
            clouds.append(c)
        pts = batch_points(clouds, stride)
        torch.cuda.synchronize()  # (the upload ran on torch's default stream)
        origins = np.array([(odoms[k][0], odoms[k][1], 0.0) for k in range(K)], dtype=np.float32)
        with torch.cuda.stream(stream):
            sh0 = segs[0].move_maps(odoms, poses, slots=slots, on_torch_stream=True)
            outs[0] = segs[0].filter_batch(pts, [len(c) for c in clouds], origins, np.full(K, -1.73), slots=slots, out=outs[0])
        sh1 = [segs[1].map(s).move(odoms[k][0], odoms[k][1], tuple(poses[k])) for k, s in enumerate(slots)]
        outs[1] = segs[1].filter_batch(pts, [len(c) for c in clouds], origins, np.full(K, -1.73), slots=slots, out=outs[1])
        torch.cuda.synchronize()
        assert [tuple(v) for v in sh0] == [tuple(v) for v in sh1], step
        got, want = outs[0].labels.cpu().numpy(), outs[1].labels.cpu().numpy()
        for k, c in enumerate(clouds):  # (the rows behind a cloud's points are not written)
            assert np.array_equal(got[k, : len(c)], want[k, : len(c)]), (step, k)
    for s in range(n_slots):
        assert_layers_equal(segs[0].map(s).layers(), segs[1].map(s).layers(), f"slot {s}")
    for seg in segs:
        seg.close()


def test_errors_change_nothing():
    (seg, other), init = two_contexts(120.0, 0.33, 6, seed=3)
    other.close()
    before = {s: (seg.map(s).layers(["ground", "groundpatch"]), seg.map(s).getPosition()) for s in range(6)}
    odoms, poses = moves_for(init, [1, 2, 3], k0=1)
    with pytest.raises(api.GroundGridError, match="GG_ERR_INVALID"):
        seg.move_maps(odoms, poses, slots=[1, 3, 1])
    with pytest.raises(api.GroundGridError, match="GG_ERR_CAPACITY"):
        seg.move_maps(odoms, poses, slots=[1, 2, 6])
    with pytest.raises(api.GroundGridError, match="GG_ERR_CAPACITY"):
        seg.move_maps(odoms, poses, slots=[-1, 2, 3])
    with pytest.raises(api.GroundGridError, match="GG_ERR_CAPACITY"):
        seg.move_maps(odoms, poses, first_slot=4)
    assert seg.move_maps(np.zeros((0, 2)), np.zeros((0, 7))).shape == (0, 2)
    for s in range(6):
        got = seg.map(s).layers(["ground", "groundpatch"])
        assert_layers_equal(got, before[s][0], f"slot {s}")
        assert lib_pos(seg, s) == before[s][1] == init[s][2]
    seg.close()
