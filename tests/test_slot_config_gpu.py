"""Per-map configuration (gg_set_slot_configs) on the device: every slot with its own configuration gives bit for bit what the CPU
oracle gives under that configuration -- one oracle.OracleMap per slot, its `cfg` set to the slot's -- in mixed batches, in every launch
shape, through every single-slot entry point and the stages, and over a scrolled fleet drive."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.test_gpu_parity import _batch_inputs, assert_same_state  # noqa: E402
from tests.test_move_maps_gpu import _drive, _pose, assert_same_as_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
ORIGIN0 = (0.0, 0.0, 0.0)


def _edit_ring40(c):
    c.max_ring = 40
    c.outlier_tolerance = 0.05
    c.min_outlier_detection_ground_confidence = 0.8


def _edit_exact_decay_near0(c):
    c.occupied_cells_decrease_factor = 1.1  # (< 1.25: the sweep's exact divide)
    c.patch_size_change_distance = 0.0
    c.point_count_cell_variance_threshold = 3


def _edit_decay3_near_all(c):
    c.occupied_cells_decrease_factor = 3.0
    c.patch_size_change_distance = 1e3
    c.distance_factor = 0.002


def _edit_labels(c):
    c.miminum_point_height_threshold = 0.2
    c.minimum_point_height_obstacle_threshold = 0.05
    c.minimum_distance_factor = 0.0008
    c.outlier_tolerance = 0.2


def _edit_absurd_count(c):
    c.ground_patch_detection_minimum_point_count_threshold = 1e9  # (every threshold >= 2^24: the +inf rule)
    c.occupied_cells_point_count_factor = 7.0


EDITS = [_edit_ring40, _edit_exact_decay_near0, _edit_decay3_near_all, _edit_labels, _edit_absurd_count]


def make_cfg(edit):
    c = api.default_config()
    if edit:
        edit(c)
    return c


def to_oracle(cfg):
    o = oracle.default_config()
    for name, _ in _lib.GGConfig._fields_:
        setattr(o, name, getattr(cfg, name))
    return o


def assign(n_slots, follow_every=3):
    """slot -> index into EDITS, or None (follows the context): every `follow_every`-th slot follows"""
    return [None if s % follow_every == 0 else (s - 1 - s // follow_every) % len(EDITS) for s in range(n_slots)]


def set_slots(seg, plan):
    own = [s for s, e in enumerate(plan) if e is not None]
    if own:
        seg.set_slot_configs([make_cfg(EDITS[plan[s]]) for s in own], slots=own)


def refs_for(plan, slots, context_cfg=None, length=120.0, res=0.33):
    refs = []
    for s in slots:
        r = oracle.OracleMap(length, res)
        r.cfg = to_oracle(make_cfg(EDITS[plan[s]]) if plan[s] is not None else (context_cfg or api.default_config()))
        refs.append(r)
    return refs


def check_batch(seg, clouds, slots, refs, frames, layer_positions, origins=None, base_z=None, tag="", stride=None):
    import torch

    B = len(clouds)
    stride = stride or (max(len(c) for c in clouds) + 63) // 64 * 64
    pts = _batch_inputs(16, clouds, stride)
    origins = np.zeros((B, 3), np.float32) if origins is None else origins
    base_z = np.full(B, -1.73) if base_z is None else base_z
    out = None
    for frame in range(frames):
        out = seg.filter_batch(pts, [len(c) for c in clouds], origins, base_z, slots=slots, out=out)
        torch.cuda.synchronize()
        labels, index, counts = out.labels.cpu().numpy(), out.out_index.cpu().numpy(), out.counts.cpu().numpy()
        for b, c in enumerate(clouds):
            r = refs[b].filter_cloud(c, tuple(origins[b]), float(base_z[b]))
            n = len(c)
            assert np.array_equal(labels[b, :n], r["label"]), (tag, frame, b, int((labels[b, :n] != r["label"]).sum()))
            assert np.array_equal(index[b, :n], r["index"]), (tag, frame, b)
            assert counts[b, 0] == len(r["out_points"]), (tag, frame, b)
            assert counts[b, 3] == (r["cls"] == oracle.OUTLIER).sum(), (tag, frame, b)
            if b in layer_positions:
                assert_same_state(seg.map(slots[b]), refs[b], f"{tag} frame {frame} cloud {b} slot {slots[b]}")


def clouds_of(count, seed0, n_az=(110, 700)):
    return [synth.hdl64_cloud(seed=seed0 + k, n_az=(n_az[1] if k % 5 == 2 else n_az[0] + 7 * (k % 4))) for k in range(count)]


# ---------------------------------------------------------------- 1. a mixed batch, bit-exact, several frames, a slot permutation

def test_mixed_batch_bit_exact():
    n_slots = 13
    plan = assign(n_slots)
    assert len({e for e in plan if e is not None}) == len(EDITS)
    clouds = clouds_of(12, 5000)
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=stride)
    set_slots(seg, plan)
    slots = [7, 1, 12, 4, 0, 9, 2, 11, 5, 3, 10, 8]  # (slot 6 stays out of the batch)
    refs = refs_for(plan, slots)
    check_batch(seg, clouds, slots, refs, 3, set(range(12)), tag="mixed")
    # the configurations reached the path: ring 40 ignores returns, the absurd count threshold never lets a cell through
    c40 = slots.index(next(s for s in slots if plan[s] == 0))
    assert (refs[c40].filter_cloud(clouds[c40])["cls"] == oracle.IGNORED).sum() > 0
    seg.close()


def test_own_config_equal_to_the_context_changes_nothing():
    """a slot whose own configuration equals the context's computes what a following slot computes (the derived constants agree)"""
    import torch

    clouds = clouds_of(6, 5100)
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    segs = [api.GroundSegmentation().init(120.0, 0.33, n_slots=6, max_points=stride) for _ in range(2)]
    segs[1].set_slot_configs([api.default_config()] * 6)
    pts = _batch_inputs(16, clouds, stride)
    outs = []
    for seg in segs:
        for _ in range(2):
            o = seg.filter_batch(pts, [len(c) for c in clouds], np.zeros((6, 3), np.float32), np.full(6, -1.73))
        torch.cuda.synchronize()
        outs.append(o.labels.cpu().numpy())
    for b, c in enumerate(clouds):  # (a row's bytes beyond its cloud are not written)
        assert np.array_equal(outs[0][b, : len(c)], outs[1][b, : len(c)]), b
    for s in range(6):
        a, b = segs[0].map(s).layers(), segs[1].map(s).layers()
        for name in a:
            assert np.array_equal(a[name], b[name], equal_nan=True), (s, name)
    for seg in segs:
        seg.close()


# ---------------------------------------------------------------- 2. launch shapes

@pytest.mark.parametrize("count", [6, 100, 288])
def test_launch_shapes(count):
    """6 clouds: the pair sweep; 100: k_sweep cut into parts; 288: the throughput k_sweep (2048-point chunks, sampled layers)"""
    plan = assign(count)
    clouds = clouds_of(count, 6000 + count, n_az=(90, 400))
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=count, max_points=stride)
    set_slots(seg, plan)
    slots = list(range(count))
    refs = refs_for(plan, slots)
    sampled = set(range(count)) if count <= 6 else set(range(0, count, 11)) | {1, 2, count - 1}
    check_batch(seg, clouds, slots, refs, 2, sampled, tag=f"{count} clouds")
    seg.close()


def test_fresh_maps_after_reset_maps():
    import torch

    count = 24  # (> 16 fresh maps: the FRESH sweep takes them as they are)
    plan = assign(count)
    clouds = clouds_of(count, 6500, n_az=(90, 300))
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=count, max_points=stride)
    set_slots(seg, plan)
    seg.reset_maps(odom_z=0.0)
    torch.cuda.synchronize()
    slots = list(range(count))
    check_batch(seg, clouds, slots, refs_for(plan, slots), 2, set(range(0, count, 2)), tag="fresh")
    seg.close()


def test_concurrent_halves():
    count = 20
    plan = assign(count)
    clouds = clouds_of(count, 6700, n_az=(90, 300))
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=count, max_points=stride)
    seg.set_flags(concurrent_halves=True)
    seg.debug_set_tuning("halves_min_clouds", 4)
    set_slots(seg, plan)
    slots = list(range(count))[::-1]
    check_batch(seg, clouds, slots, refs_for(plan, slots), 2, set(range(0, count, 3)), tag="halves")
    seg.close()


@pytest.mark.parametrize("eager", [False, True])
def test_eager_and_lazy_layers(eager):
    count = 8
    plan = assign(count)
    clouds = clouds_of(count, 6800)
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=count, max_points=stride)
    seg.set_flags(eager_layers=eager)
    set_slots(seg, plan)
    slots = list(range(count))
    check_batch(seg, clouds, slots, refs_for(plan, slots), 2, set(range(count)), tag=f"eager={eager}")
    seg.close()


def test_big_map_1000():
    length, res = 330.0, 0.33
    count = 4
    plan = [None, 1, 2, 4]
    clouds = [synth.hdl64_cloud(seed=6900 + k, n_az=300) for k in range(count)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(length, res, n_slots=count, max_points=stride)
    assert seg.rows == 1000
    set_slots(seg, plan)
    slots = list(range(count))
    check_batch(seg, clouds, slots, refs_for(plan, slots, length=length, res=res), 2, set(range(count)), tag="1000^2")
    seg.close()


@pytest.mark.parametrize("knob", ["pw2048", "sweep_waves1", "sweep_waves2", "sweep_waves3", "k2_per_cloud64", "k2_dense_share4", "all_big_batch",
                                  "sweep_pair_off", "sweep_pair_batch"])
def test_each_launch_geometry_switch(knob, monkeypatch):
    """the switches of test_gpu_parity.py::test_each_launch_geometry_switch_forced_at_small_batch, and the pair sweeps off / on the
    layer in place (a launch with clouds of their own configuration keeps k_sweep there)"""
    if knob in ("pw2048", "all_big_batch"):
        monkeypatch.setenv("GG_PW", "2048")
    clouds = [synth.hdl64_cloud(seed=410 + k, n_az=n) for k, n in enumerate([2083, 700, 150, 1200, 90])] + [synth.empty_cloud(0)]
    B, stride = len(clouds), (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    if knob in ("pw2048", "all_big_batch"):
        assert seg.debug_set_tuning("pw", 0) == 2048
    if knob.startswith("sweep_waves"):
        seg.debug_set_tuning("sweep_waves", int(knob[-1]))
    if knob in ("k2_per_cloud64", "all_big_batch"):
        seg.debug_set_tuning("k2_per_cloud", 64)
    if knob == "k2_dense_share4":
        seg.debug_set_tuning("k2_dense_share", 4)
    if knob == "all_big_batch":
        seg.debug_set_tuning("sweep_waves", 2)
    if knob == "sweep_pair_off":
        seg.debug_set_tuning("sweep_pair", 2)
    if knob == "sweep_pair_batch":
        seg.debug_set_tuning("sweep_pair", 4)
    plan = [1, None, 0, 2, 3, 4]
    set_slots(seg, plan)
    slots = list(range(B))
    check_batch(seg, clouds, slots, refs_for(plan, slots), 3, set(range(B)), tag=knob)
    seg.close()


# ---------------------------------------------------------------- 3. single-slot entry points and stages

def _single_pair(edit, n_slots=3, slot=1):
    cloud = synth.hdl64_cloud(seed=71, n_az=500)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n_slots, max_points=len(cloud))
    cfg = make_cfg(edit)
    seg.map(slot).setConfig(cfg)
    ref = oracle.OracleMap(120.0, 0.33)
    ref.cfg = to_oracle(cfg)
    return seg, ref, cloud, seg.map(slot)


def _assert_frame(seg, ref, m, got_labels, got_index, r, tag):
    assert np.array_equal(got_labels, r["label"]), tag
    assert np.array_equal(got_index, r["index"]), tag
    assert_same_state(m, ref, tag)


@pytest.mark.parametrize("edit", [0, 1, 2, 3, 4])
def test_filter_cloud_with_and_without_transform(edit):
    seg, ref, cloud, m = _single_pair(EDITS[edit])
    for f in range(2):
        _, labels, index = seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m, return_details=True)
        _assert_frame(seg, ref, m, labels, index, ref.filter_cloud(cloud, ORIGIN0, -1.73), f"plain {f}")
    tf = np.array([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 0.0]], dtype=np.float64)
    moved = synth.clone_cloud(cloud)
    moved["x"] += np.float32(0.5)
    moved["y"] -= np.float32(0.25)
    _, labels, index = seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m, return_details=True, map_from_cloud=tf)
    _assert_frame(seg, ref, m, labels, index, ref.filter_cloud(moved, ORIGIN0, -1.73), "tf")
    seg.close()


def test_filter_cloud_with_layers_async_and_graphs():
    seg, ref, cloud, m = _single_pair(_edit_decay3_near_all)
    planes = seg.alloc_layers()
    _, labels, index = seg.filter_cloud_with_layers(cloud, ORIGIN0, -1.73, planes, map=m, return_details=True)
    r = ref.filter_cloud(cloud, ORIGIN0, -1.73)
    _assert_frame(seg, ref, m, labels, index, r, "with layers")
    for name in oracle.LAYERS:
        assert np.array_equal(planes[name], ref.layer(name), equal_nan=True), name
    seg.release_layers(planes)
    t = seg.filter_cloud_async(cloud, ORIGIN0, -1.73, map=m)
    _, labels, index = seg.filter_cloud_wait(t, return_details=True)
    _assert_frame(seg, ref, m, labels, index, ref.filter_cloud(cloud, ORIGIN0, -1.73), "async")
    seg.debug_set_tuning("graphs", 1)
    for f in range(3):  # (eager, captured, replayed)
        _, labels, index = seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m, return_details=True)
        _assert_frame(seg, ref, m, labels, index, ref.filter_cloud(cloud, ORIGIN0, -1.73), f"graph {f}")
    seg.close()


def test_filter_cloud_pc2_out_matches_a_context_with_that_configuration():
    seg, ref, cloud, m = _single_pair(_edit_ring40)
    twin = api.GroundSegmentation().init(120.0, 0.33, n_slots=3, max_points=len(cloud))
    twin.setConfig(make_cfg(_edit_ring40))
    data = api.to_pc2(cloud)
    offsets = (0, 4, 8, 16)
    for f in range(2):
        got = seg.filter_cloud_pc2_out(data.tobytes(), len(cloud), 18, offsets, ORIGIN0, -1.73, map=m)
        want = twin.filter_cloud_pc2_out(data.tobytes(), len(cloud), 18, offsets, ORIGIN0, -1.73, map=twin.map(1))
        assert np.array_equal(got, want), f
        ref.filter_cloud(cloud, ORIGIN0, -1.73)
        assert_same_state(m, ref, f"pc2 {f}")
    seg.close()
    twin.close()


def test_insert_cloud_and_every_stage():
    seg, ref, cloud, m = _single_pair(_edit_ring40)
    seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m)
    ref.filter_cloud(cloud, ORIGIN0, -1.73)
    low = synth.clone_cloud(cloud)
    low["z"][::3] -= np.float32(0.9)
    cls, cell = m.insert_cloud(low, 0, len(low), (0.5, -0.25, 0.1))
    rcls, _ = ref.stage_insert(low, (0.5, -0.25, 0.1))
    assert np.array_equal(cls, rcls)
    assert (rcls == oracle.IGNORED).sum() > 0
    assert_same_state(m, ref, "insert")
    m.detect_ground_patches(1)
    ref.stage_detect_section(1)
    m.detect_ground_patches(-1)
    ref.stage_detect()
    assert_same_state(m, ref, "detect")
    seg.close()

    seg, ref, cloud, m = _single_pair(_edit_exact_decay_near0)
    seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m)
    ref.filter_cloud(cloud, ORIGIN0, -1.73)
    m.detect_ground_patches(-1)
    ref.stage_detect()
    m.spiral_ground_interpolation(-1.5)
    ref.stage_spiral(-1.5)
    assert_same_state(m, ref, "spiral")
    rng = np.random.default_rng(3)
    n = ref.rows
    for _ in range(20):
        S = int(rng.choice([3, 5]))
        i, j = (int(v) for v in rng.integers(S // 2 + 150, n - S // 2 - 150, 2))
        m.detect_ground_patch(S, i, j)
        ref.detect_ground_patch(S, i, j)
        x, y = (int(v) for v in rng.integers(1, n - 1, 2))
        m.interpolate_cell(x, y)
        ref.interpolate_cell(x, y)
    assert_same_state(m, ref, "cells")
    seg.close()


# ---------------------------------------------------------------- 4. semantics

def test_semantics_follow_keep_clear_and_report():
    import torch

    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=64)
    own = make_cfg(_edit_labels)
    seg.set_slot_configs([own], slots=[2])
    c, o = seg.slot_config(2)
    assert o and c.miminum_point_height_threshold == own.miminum_point_height_threshold
    c, o = seg.slot_config(1)
    assert not o and c.max_ring == api.default_config().max_ring
    ctx_cfg = make_cfg(_edit_ring40)
    seg.setConfig(ctx_cfg)
    assert seg.slot_config(1)[0].max_ring == 40 and not seg.slot_config(1)[1]    # following slots follow later gg_set_config calls
    assert seg.slot_config(2)[0].max_ring == own.max_ring and seg.slot_config(2)[1]
    assert seg.getConfig().max_ring == 40                                        # gg_get_config: the context's
    seg.map(2).reset()
    seg.reset_maps()
    seg.move_maps([(3.0, 1.0)], [(0, 0, 0, 0, 0, 0, 1)], slots=[2])
    torch.cuda.synchronize()
    assert seg.slot_config(2)[1]                                                 # kept through resets and moves
    seg.map(2).setConfig(None)
    c, o = seg.slot_config(2)
    assert not o and c.max_ring == 40
    # errors change nothing
    seg.set_slot_configs([own, own], slots=[0, 3])
    with pytest.raises(api.GroundGridError):
        seg.set_slot_configs([ctx_cfg, ctx_cfg], slots=[1, 4])                  # outside the context
    with pytest.raises(api.GroundGridError):
        seg.set_slot_configs([ctx_cfg, ctx_cfg], slots=[1, 1])                  # a duplicate
    with pytest.raises(api.GroundGridError):
        seg.set_slot_configs([ctx_cfg] * 2, first_slot=3)
    assert [seg.slot_config(s)[1] for s in range(4)] == [True, False, False, True]
    assert seg.slot_config(0)[0].minimum_point_height_obstacle_threshold == own.minimum_point_height_obstacle_threshold
    L = seg._L
    cfg = _lib.GGConfig()
    assert L.gg_set_slot_configs(seg._ctx, -1, None, 0, None) == -1
    assert L.gg_set_slot_configs(seg._ctx, 1, (C.c_int32 * 1)(-1), 0, C.byref(cfg)) == -5
    assert L.gg_get_slot_config(seg._ctx, 4, C.byref(cfg), None) == -5
    seg.set_slot_configs(None, slots=[0, 3])
    assert not any(seg.slot_config(s)[1] for s in range(4))
    seg.close()


def test_a_batch_enqueued_before_the_change_uses_the_old_settings():
    import torch

    clouds = clouds_of(4, 7100)
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=4, max_points=stride)
    pts = _batch_inputs(16, clouds, stride)
    plan = [None] * 4
    refs = refs_for(plan, range(4))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = seg.filter_batch(pts, [len(c) for c in clouds], np.zeros((4, 3), np.float32), np.full(4, -1.73))
        seg.set_slot_configs([make_cfg(_edit_ring40)] * 4)   # (blocks until the batch above has finished)
        labels = out.labels.cpu().numpy()
    for b, c in enumerate(clouds):
        r = refs[b].filter_cloud(c, ORIGIN0, -1.73)
        assert np.array_equal(labels[b, : len(c)], r["label"]), b
    for r in refs:  # the maps as the first batch left them, under the new configuration from here on
        r.cfg = to_oracle(make_cfg(_edit_ring40))
    check_batch(seg, clouds, list(range(4)), refs, 1, set(range(4)), tag="after")
    seg.close()


def test_graph_replay_sees_a_config_change():
    seg, ref, cloud, m = _single_pair(None)
    seg.debug_set_tuning("graphs", 1)
    for f in range(3):
        _, labels, index = seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m, return_details=True)
        _assert_frame(seg, ref, m, labels, index, ref.filter_cloud(cloud, ORIGIN0, -1.73), f"before {f}")
    for edit in (_edit_ring40, _edit_labels, None):
        cfg = make_cfg(edit)
        m.setConfig(cfg if edit else None)
        ref.cfg = to_oracle(cfg)
        for f in range(3):
            _, labels, index = seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m, return_details=True)
            _assert_frame(seg, ref, m, labels, index, ref.filter_cloud(cloud, ORIGIN0, -1.73), f"{edit} {f}")
    seg.close()


# ---------------------------------------------------------------- 5. a parameter sweep over a scrolled drive

def test_parameter_sweep_drive():
    import torch

    K, frames = 8, 30
    path = _drive(2, frames)[1]                   # ONE drive (moving and turning), replayed by K candidate configurations in lockstep
    edits = EDITS + [None, _edit_ring40, _edit_absurd_count]
    cfgs = [make_cfg(e) for e in edits]
    cfgs[6].outlier_tolerance = 0.3
    cfgs[7].ground_patch_detection_minimum_point_count_threshold = 0.5
    base = [synth.hdl64_cloud(seed=950 + v, n_az=120) for v in range(3)]
    stride = (max(len(c) for c in base) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=K, max_points=stride)
    seg.set_slot_configs(cfgs)
    refs = [oracle.OracleMap(120.0, 0.33) for _ in range(K)]
    for v in range(K):
        refs[v].cfg = to_oracle(cfgs[v])
    out = None
    for f in range(frames):
        x, y, th = path[f]
        c = synth.clone_cloud(base[f % 3])
        c["x"] += np.float32(x)
        c["y"] += np.float32(y)
        clouds = [c] * K
        origins = np.array([(x, y, 0.0)] * K, dtype=np.float32)
        odoms = np.array([(x, y)] * K)
        poses = np.array([_pose(x, y, th)] * K, dtype=np.float64)
        seg.move_maps(odoms, poses)
        out = seg.filter_batch(_batch_inputs(16, clouds, stride), [len(c)] * K, origins, np.full(K, -1.73), out=out)
        torch.cuda.synchronize()
        labels = out.labels.cpu().numpy()
        for v in range(K):
            refs[v].update(x, y, poses[v])
            r = refs[v].filter_cloud(c, (x, y, 0.0), -1.73)
            assert np.array_equal(labels[v, : len(c)], r["label"]), (f, v)
    for v in range(K):
        assert_same_as_oracle(seg.map(v), refs[v], f"candidate {v}")
    seg.close()
