"""The evaluator counters on the device (gg_set_slot_scoring / gg_get_slot_scores, k8_score.hip).  The expected value is always
GroundEvaluator.add_cloud fed with what the ORACLE returned for that map (oracle.OracleMap.filter_cloud: the returned cloud, whose
intensity is the label and whose ring is the id) -- never anything read back from the device path.  Every comparison is integer
equality of every counter of every slot, the cloud count included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, kitti, replay, synth  # noqa: E402
from groundgrid_amd.evaluate import LABELS, GroundEvaluator  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import edge_scenes as es  # noqa: E402
from tests.test_gpu_batch_edges import Run, _layout, _with_edges_of_the_stride  # noqa: E402
from tests.test_gpu_parity import _batch_inputs  # noqa: E402
from tests.test_kitti_cpu import OracleBackend  # noqa: E402
from tests.test_slot_config_gpu import EDITS, make_cfg, to_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
ORIGIN0 = (0.0, 0.0, 0.0)
LENGTH, RES = 120.0, 0.33
IDS = list(LABELS.keys())


def add_returned(ev, r):
    """the reference's callback on the cloud the oracle returned: intensity = prediction, ring = label id, skip_nans on x, y, z"""
    out = r["out_points"]
    ev.add_cloud(out["intensity"].astype(np.uint8), out["ring"], points=out, allow_unknown=True)


def zero():
    return GroundEvaluator().counters()


def device_counters(seg, slots=None, **kw):
    return [e.counters() for e in seg.scores(slots=slots, allow_unknown=True, **kw)]


def all_ids_cloud(seed=3):
    """every listed id and 65535, each on ground-like and on raised points"""
    c = synth.hdl64_cloud(seed=seed, n_az=150)
    ids = np.array(IDS + [65535], dtype=np.uint16)
    c["ring"] = ids[np.arange(len(c)) % len(ids)]
    return c


class Recording:
    """an oracle map that also feeds an evaluator with every cloud it returns"""

    def __init__(self, ref, scoring=True):
        self.__dict__["ref"], self.__dict__["ev"], self.__dict__["scoring"] = ref, GroundEvaluator(), scoring

    def filter_cloud(self, *a, **k):
        r = self.ref.filter_cloud(*a, **k)
        if self.scoring:
            add_returned(self.ev, r)
        return r

    def __getattr__(self, name):
        return getattr(self.ref, name)

    def __setattr__(self, name, value):
        setattr(self.ref, name, value)


def record(run, scoring_slots):
    run.seg.set_score_labels()
    run.seg.set_scoring(slots=sorted(scoring_slots))
    run.refs = [Recording(r, s in scoring_slots) for s, r in enumerate(run.refs)]


def assert_scores(run, tag):
    got = device_counters(run.seg)
    for s, rec in enumerate(run.refs):
        assert got[s] == rec.ev.counters(), f"{tag}: slot {s} ({run.at[s].name})"


# ---------------------------------------------------------------- 1. a mixed batch

@pytest.mark.parametrize("fmt,transforms", [(16, False), (32, False), (16, True), (32, True)])
def test_mixed_batch_of_scoring_and_other_slots(fmt, transforms):
    n_slots = 24
    clouds = [synth.hdl64_cloud(seed=8000 + k, n_az=110 + 7 * (k % 4)) for k in range(n_slots - 1)] + [all_ids_cloud()]  # ring = beam 0..63
    scenes = [es.Scene(f"beam_{k}", c, "filler") for k, c in enumerate(clouds)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    slots = np.random.default_rng(11).permutation(n_slots).astype(np.int32)
    run = Run(n_slots, scenes, slots, stride, fmt=fmt, transforms=transforms)
    scoring = {s for s in range(n_slots) if s % 3 != 0} | {n_slots - 1}
    record(run, scoring)
    for f in range(3):
        run.step(f"mixed/{fmt}/{transforms} frame {f}", extras=(f == 2))  # (extras: the caller's own d_label_masks)
    assert_scores(run, "mixed")
    got = device_counters(run.seg)
    for s in range(n_slots):
        if s not in scoring:
            assert got[s] == zero(), s
    last = run.refs[n_slots - 1].ev
    assert last.unknown_total > 0 and all(last.total[n] > 0 for n in LABELS.values()) and last.cloud_count == 3
    assert run.refs[1].ev.unknown_total > 0 and run.refs[1].ev.total["road"] > 0  # beams 0..63: listed ids and the other bin
    with pytest.raises(KeyError):
        run.seg.scores(slots=[n_slots - 1])
    run.close()


# ---------------------------------------------------------------- 2. launch shapes

@pytest.mark.parametrize("count", [1, 16, 17, 288])
def test_launch_shapes(count):
    clouds = [synth.hdl64_cloud(seed=8100 + k, n_az=(400 if k % 5 == 2 else 90 + 5 * (k % 4))) for k in range(count)]
    clouds[0] = all_ids_cloud(5)
    scenes = [es.Scene(f"c{k}", c, "filler") for k, c in enumerate(clouds)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    cfgs = {s: make_cfg(EDITS[s % len(EDITS)]) for s in range(count) if s % 4 == 1}  # per-slot configurations mixed in
    run = Run(count, scenes, None, stride, slot_cfgs=cfgs)
    record(run, {s for s in range(count) if s % 5 != 3})
    for f in range(2):
        run.step(f"{count} clouds frame {f}")
    assert_scores(run, f"{count} clouds")
    run.close()


def test_257_fresh_maps():
    B = 257
    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, B - len(hostile), 8200)
    at, slots = _layout(B, hostile, fill, permute=False, seed=3)
    run = Run(B, at, slots, stride, fresh=True)
    record(run, set(range(B)) - {5, 100})
    assert run.seg.debug_set_tuning("fresh_count", 0) == B
    assert device_counters(run.seg, slots=[0, 256]) == [zero(), zero()]  # a getter in between ...
    assert run.seg.debug_set_tuning("fresh_count", 0) == B               # ... leaves the maps fresh
    run.step("fresh")
    assert run.seg.debug_set_tuning("fresh_count", 0) == 0
    run.step("warm")
    assert_scores(run, "257 fresh")
    run.close()


@pytest.mark.parametrize("fence", [True, False])
def test_concurrent_halves(fence):
    import torch

    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, 24 - len(hostile), 8300)
    at, slots = _layout(24, hostile, fill, permute=True, seed=4)
    run = Run(24, at, slots, stride, halves=True, tuning=[("halves_min_clouds", 2)])
    record(run, set(range(24)) - {2, 13})
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for f in range(2):
            run.step(f"halves frame {f}")
        # one more batch, and the getter straight behind it: it orders itself after both halves
        run.seg.filter_batch(run.pts, run.n, run.origins, run.base_z, slots=run.slots, out=run.out)
        if fence:
            run.seg.batch_fence()
        got = device_counters(run.seg)
    for b, s in enumerate(run.cloud_slot):
        run.refs[s].filter_cloud(run.map_clouds[b], tuple(float(v) for v in run.origins[b]), float(run.base_z[b]))
    for s, rec in enumerate(run.refs):
        assert got[s] == rec.ev.counters(), (fence, s, at[s].name)
    side.synchronize()
    run.close()


@pytest.mark.parametrize("knob,value", [("k2_dense_share", 4), ("sweep_waves", 1), ("sweep_waves", 3), ("front", 1), ("front", 2), ("front", 3),
                                        ("sweep_pair", 2), ("sweep_pair", 4)])
def test_forced_launch_tunings(knob, value):
    hostile = es.adversarial_scenes()
    n = 12 if knob == "sweep_pair" else 24
    hostile = hostile[: n - 4]
    fill, stride = _with_edges_of_the_stride(hostile, n - len(hostile), 8400)
    at, slots = _layout(n, hostile, fill, permute=(value % 2 == 1), seed=6)
    run = Run(n, at, slots, stride, tuning=[(knob, value)])
    record(run, set(range(n)) - {3})
    for f in range(2):
        run.step(f"{knob}={value} frame {f}")
    assert_scores(run, f"{knob}={value}")
    run.close()


# ---------------------------------------------------------------- 3. hostile scenes, single calls and batched; every single-cloud entry point

def test_hostile_scenes_as_single_calls():
    nan_skipped = 0
    for sc in es.adversarial_scenes():
        seg = api.GroundSegmentation().init(sc.length, sc.resolution, n_slots=2, max_points=max(len(sc.cloud), 1))
        seg.map(1).reset(odom_z=sc.odom_z, pos=sc.pos)
        seg.set_scoring(slots=[1])
        ref = oracle.OracleMap(sc.length, sc.resolution, pos=sc.pos, odom_z=sc.odom_z)
        ev = GroundEvaluator()
        for f in range(sc.frames):
            _, labels, index = seg.filter_cloud(sc.cloud, sc.origin, sc.base_z, map=seg.map(1), return_details=True)
            r = ref.filter_cloud(sc.cloud, tuple(float(v) for v in sc.origin), sc.base_z)
            assert np.array_equal(labels, r["label"]) and np.array_equal(index, r["index"]), (sc.name, f)
            add_returned(ev, r)
            nan_skipped += int(np.isnan(r["out_points"]["z"]).sum())
        assert device_counters(seg) == [zero(), ev.counters()], sc.name
        assert seg.map(1).scores(allow_unknown=True).counters() == ev.counters()
        seg.close()
    assert nan_skipped > 0


@pytest.mark.parametrize("fmt", [16, 32])
def test_hostile_scenes_batched(fmt):
    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, 24 - len(hostile), 8500)
    at, slots = _layout(24, hostile, fill, permute=True, seed=1)
    run = Run(24, at, slots, stride, fmt=fmt)
    record(run, set(range(24)))
    for f in range(3):
        run.step(f"hostile/{fmt} frame {f}")
    assert_scores(run, f"hostile/{fmt}")
    run.close()


def test_every_single_cloud_entry_point():
    cloud = all_ids_cloud(9)
    cloud["z"][7] = np.nan
    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=3, max_points=len(cloud))
    m = seg.map(1)
    seg.set_scoring(slots=[1])
    ref, ev = oracle.OracleMap(LENGTH, RES), GroundEvaluator()

    def expect(c=cloud):
        add_returned(ev, ref.filter_cloud(c, ORIGIN0, -1.73))
        assert device_counters(seg, slots=[1]) == [ev.counters()]

    seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m)
    expect()
    tf = np.array([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 0.0]], dtype=np.float64)
    moved = kitti.transform_cloud(cloud, tf[:, :3], tf[:, 3])  # (the NaN height makes the transformed point NaN all over: dropped)
    seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m, map_from_cloud=tf)
    expect(moved)
    t0 = seg.filter_cloud_async(cloud, ORIGIN0, -1.73, map=m)
    t1 = seg.filter_cloud_async(cloud, ORIGIN0, -1.73, map=m, map_from_cloud=tf)
    seg.filter_cloud_wait(t0)
    seg.filter_cloud_wait(t1)
    add_returned(ev, ref.filter_cloud(cloud, ORIGIN0, -1.73))
    expect(moved)
    planes = seg.alloc_layers()
    seg.filter_cloud_with_layers(cloud, ORIGIN0, -1.73, planes, map=m)
    seg.release_layers(planes)
    expect()
    # PointCloud2 payloads with the ring somewhere else than the player puts it: x@4 y@8 z@12 ring@2, 20-byte records
    dt = np.dtype({"names": ["ring", "x", "y", "z"], "formats": ["<u2", "<f4", "<f4", "<f4"], "offsets": [2, 4, 8, 12], "itemsize": 20})
    data = np.zeros(len(cloud), dtype=dt)
    for k in ("ring", "x", "y", "z"):
        data[k] = cloud[k]
    seg.filter_cloud_pc2(data.tobytes(), len(cloud), 20, (4, 8, 12, 2), ORIGIN0, -1.73, map=m)
    expect()
    seg.filter_cloud_pc2_out(data.tobytes(), len(cloud), 20, (4, 8, 12, 2), ORIGIN0, -1.73, map=m, map_from_cloud=tf)
    expect(moved)
    seg.debug_set_tuning("graphs", 1)
    for _ in range(3):  # eager, captured, replayed
        seg.filter_cloud(cloud, ORIGIN0, -1.73, map=m)
        expect()
    # insert_cloud and the stages do not label and do not score
    m.insert_cloud(cloud, 0, len(cloud), ORIGIN0)
    m.detect_ground_patches(-1)
    assert device_counters(seg, slots=[1]) == [ev.counters()] and ev.cloud_count == 10
    assert device_counters(seg, slots=[0, 2]) == [zero(), zero()]
    seg.close()


# ---------------------------------------------------------------- 4. lifetime and errors

def test_lifetime_of_the_counters():
    import torch

    clouds = [all_ids_cloud(20 + k) for k in range(4)]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=4, max_points=stride)
    seg.set_scoring()
    refs = [oracle.OracleMap(LENGTH, RES) for _ in range(4)]
    evs = [GroundEvaluator() for _ in range(4)]
    on = [True] * 4
    pts = _batch_inputs(16, clouds, stride)

    def step():
        seg.filter_batch(pts, [len(c) for c in clouds], np.zeros((4, 3), np.float32), np.full(4, -1.73))
        torch.cuda.synchronize()
        for b in range(4):
            r = refs[b].filter_cloud(clouds[b], ORIGIN0, -1.73)
            if on[b]:
                add_returned(evs[b], r)
        assert device_counters(seg) == [e.counters() for e in evs]

    step()
    seg.reset_maps(odom_z=0.1)                                   # counters continue across reset_maps ...
    for r in refs:
        r.reset_state(odom_z=0.1)
    step()
    pose = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    seg.move_maps([(1.0, -0.7)] * 4, [pose] * 4)                 # ... move_maps ...
    for r in refs:
        r.update(1.0, -0.7, pose)
    step()
    cfg = make_cfg(EDITS[3])
    seg.setConfig(cfg)                                           # ... setConfig and a slot's own configuration ...
    for r in refs:
        r.cfg = to_oracle(cfg)
    seg.map(2).setConfig(make_cfg(EDITS[0]))
    refs[2].cfg = to_oracle(make_cfg(EDITS[0]))
    step()
    seg.set_scoring(slots=[1, 3], enable=False)                  # ... and off / on
    on[1] = on[3] = False
    step()
    seg.set_scoring(slots=[3])
    on[3] = True
    step()
    seg.reset_scores(slots=[2, 0])                               # zeroes only the named slots, keeps on / off
    evs[0], evs[2] = GroundEvaluator(), GroundEvaluator()
    assert device_counters(seg) == [e.counters() for e in evs]
    step()
    seg.set_score_labels(IDS[::-1])                              # a new list zeroes everything; the slots stay on / off
    evs[:] = [GroundEvaluator() for _ in range(4)]
    assert device_counters(seg) == [zero()] * 4
    step()
    assert evs[1].cloud_count == 0 and evs[0].cloud_count == 1
    seg.set_score_labels([40, 50])                               # a short list: everything else is the other bin
    step_ev = seg.scores(allow_unknown=True)
    assert all(e.counters() == zero() for e in step_ev)
    seg.filter_batch(pts, [len(c) for c in clouds], np.zeros((4, 3), np.float32), np.full(4, -1.73))
    r = refs[0].filter_cloud(clouds[0], ORIGIN0, -1.73)["out_points"]
    keep = ~np.isnan(r["z"])
    e = seg.scores(slots=[0], allow_unknown=True)[0]
    assert e.total["road"] == int(((r["ring"] == 40) & keep).sum()) and e.total["building"] == int(((r["ring"] == 50) & keep).sum())
    assert e.unknown_total == int((~np.isin(r["ring"], [40, 50]) & keep).sum()) and e.cloud_count == 1
    seg.close()


def test_error_codes_change_nothing():
    seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=4, max_points=64)
    L, ctx = seg._L, seg._ctx
    one = (C.c_int32 * 1)(0)
    out = (_lib.GGSlotScores * 4)()
    assert L.gg_set_slot_scoring(ctx, 1, None, 0, 1) == -1          # no label list yet
    assert L.gg_get_slot_scores(ctx, 1, None, 0, out) == -1
    assert L.gg_reset_slot_scores(ctx, 1, None, 0) == -1
    for bad in ([], [40, 40], [-1], [65536], list(range(65))):
        arr = (C.c_int32 * max(len(bad), 1))(*bad)
        assert L.gg_set_score_labels(ctx, len(bad), arr) == -1, bad
    assert L.gg_set_score_labels(ctx, 2, None) == -1
    assert L.gg_set_slot_scoring(ctx, 1, None, 0, 1) == -1          # ... still none
    seg.set_score_labels(list(range(64)))                            # 64 ids are fine
    seg.set_score_labels()
    seg.set_scoring(slots=[2])
    assert L.gg_set_slot_scoring(ctx, -1, None, 0, 1) == -1
    assert L.gg_set_slot_scoring(ctx, 0, None, 0, 1) == 0
    assert L.gg_set_slot_scoring(ctx, 2, (C.c_int32 * 2)(1, 4), 0, 1) == -5
    assert L.gg_set_slot_scoring(ctx, 2, (C.c_int32 * 2)(1, 1), 0, 1) == -1
    assert L.gg_set_slot_scoring(ctx, 2, None, 3, 1) == -5
    assert L.gg_get_slot_scores(ctx, 2, None, 3, out) == -5 and L.gg_get_slot_scores(ctx, 1, (C.c_int32 * 1)(-1), 0, out) == -5
    assert L.gg_get_slot_scores(ctx, 2, (C.c_int32 * 2)(3, 3), 0, out) == -1 and L.gg_get_slot_scores(ctx, 1, one, 0, None) == -1
    assert L.gg_get_slot_scores(ctx, 0, None, 0, None) == 0 and L.gg_reset_slot_scores(ctx, 0, None, 0) == 0
    assert L.gg_reset_slot_scores(ctx, 1, None, 4) == -5 and L.gg_reset_slot_scores(ctx, 2, (C.c_int32 * 2)(0, 0), 0) == -1
    # only slot 2 scores: the failed calls switched nothing on
    cloud = synth.hdl64_cloud(seed=1, n_az=1)[:64]
    for s in range(4):
        seg.filter_cloud(cloud, ORIGIN0, -1.73, map=seg.map(s))
    clouds, _ = seg.scores_raw()
    assert clouds.tolist() == [0, 0, 1, 0]
    seg.close()


# ---------------------------------------------------------------- 5. the sweep

def test_score_configs_equals_the_oracle_replayed_once_per_configuration():
    cfgs = [make_cfg(e) for e in EDITS] + [api.default_config()]
    frames = list(kitti.synthetic_drive(n_frames=40, n_az=700))
    got = replay.score_configs(frames, cfgs, max_points=max(len(f.cloud_map) for f in frames))
    assert len(got) == 6
    tables = set()
    for k, cfg in enumerate(cfgs):
        backend = OracleBackend()
        reset = backend.reset

        def reset_with_cfg(pos, odom_z, reset=reset, backend=backend, cfg=cfg):
            reset(pos, odom_z)
            backend.m.cfg = to_oracle(cfg)

        backend.reset = reset_with_cfg
        want, _ = replay.replay(frames, backend)
        assert got[k].counters() == want.counters(), k
        assert got[k].table() == want.table(), k
        assert want.cloud_count == 40
        tables.add(want.table())
    assert len(tables) > 1  # the configurations score differently: the sweep has something to choose from
