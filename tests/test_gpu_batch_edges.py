"""The hostile scenes of tests/edge_scenes.py through gg_filter_batch, at the launch shapes the throughput path takes (pytest -m gpu,
on a real MI355X).  Every cloud of a batch against its own oracle map (one per slot, with that slot's position, initial height and
configuration): labels, emission index, all four counts, per-point classes and cells; for the hostile slots and a sample of the
others also all 11 layers (lazily materialised), the returned clouds, the 18-byte PointCloud2 records and the 2-bit label masks.

The hostile clouds sit at slot 0, at the last slot, on both sides of the halves boundary and elsewhere; some cases hand them over
through a `slots=` permutation.  The rest of each batch is ordinary sensor clouds, plus clouds of stride - 1 and exactly stride
points (the last one fills its row)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from groundgrid_amd import _lib, api, kitti, synth  # noqa: E402
from groundgrid_amd.dist import pack_label_masks  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import edge_scenes as es  # noqa: E402
from tests.test_gpu_parity import _batch_inputs, _mixed_small_clouds, _rotated_clouds, assert_same_state  # noqa: E402
from tests.test_slot_config_gpu import EDITS, make_cfg, to_oracle  # noqa: E402

LENGTH, RES = 120.0, 0.33


def _fillers(count, seed0):
    """ordinary sensor clouds: distinct small ones (some ~36 k points) and rotated copies of one"""
    half = count // 2
    return _mixed_small_clouds(half, seed0) + _rotated_clouds(count - half, LENGTH, seed=seed0 + 7, n_az=110)


def _layout(n_slots, hostile, fillers, permute, seed):
    """slot -> scene: the hostile scenes on slot 0, the last slot, both sides of the halves boundary, then spread over the rest;
    fillers everywhere else.  Returns (scene per slot, slots[b] of cloud b or None for the identity)."""
    h = (n_slots + 1) // 2
    order = [0, n_slots - 1, h - 1, h]
    order += [int(s) for s in np.linspace(1, n_slots - 2, 3 * len(hostile)).round() if int(s) not in order]
    order = list(dict.fromkeys(order))[: len(hostile)]
    assert len(order) == len(hostile)
    at = [None] * n_slots
    for s, sc in zip(order, hostile):
        at[s] = sc
    it = iter(fillers)
    for s in range(n_slots):
        if at[s] is None:
            c = next(it)
            at[s] = es.Scene(f"filler_{s}", c, "filler")
    slots = np.random.default_rng(seed).permutation(n_slots).astype(np.int32) if permute else None
    return at, slots


def _with_edges_of_the_stride(hostile, n_fill, seed0, stride_floor=0):
    """fillers, a cloud of stride - 1 points and one of exactly stride points: the stride is the largest cloud rounded up to 64"""
    fill = _fillers(n_fill - 2, seed0)
    stride = (max([len(s.cloud) for s in hostile] + [len(c) for c in fill] + [stride_floor]) + 63) // 64 * 64
    fill = [es.sized(stride - 1).cloud, es.sized(stride).cloud] + fill
    return fill, stride


class Run:
    """One context and one oracle map per slot; `step` runs a batch and checks it."""

    def __init__(self, n_slots, at, slots, stride, fmt=16, fresh=False, slot_cfgs=None, transforms=False, halves=False, tuning=()):
        self.n_slots, self.at, self.slots, self.stride, self.fmt, self.halves = n_slots, at, slots, stride, fmt, halves
        self.seg = api.GroundSegmentation().init(LENGTH, RES, n_slots=n_slots, max_points=stride)
        for key, value in tuning:
            self.seg.debug_set_tuning(key, value)
        if halves:
            self.seg.set_flags(concurrent_halves=True)
        self.refs = []
        z0 = 0.25 if fresh else None
        if fresh:
            self.seg.reset_maps(odom_z=0.25)
        for s, sc in enumerate(at):
            odom_z = z0 if fresh else sc.odom_z
            if sc.pos != (0.0, 0.0) or sc.odom_z != 0.0:
                if fresh:
                    self.seg.reset_maps(first_slot=s, n_slots=1, odom_z=odom_z, pos=sc.pos)
                else:
                    self.seg.map(s).reset(odom_z=odom_z, pos=sc.pos)
            self.refs.append(oracle.OracleMap(LENGTH, RES, pos=sc.pos, odom_z=odom_z))
        if slot_cfgs:
            own = sorted(slot_cfgs)
            self.seg.set_slot_configs([slot_cfgs[s] for s in own], slots=own)
            for s in own:
                self.refs[s].cfg = to_oracle(slot_cfgs[s])
        B = n_slots
        self.cloud_slot = [int(slots[b]) if slots is not None else b for b in range(B)]
        scenes = [at[s] for s in self.cloud_slot]
        self.tfs = None
        if transforms:  # cloud b arrives in its sensor frame: map <- sensor is a rotation about the map-frame point of the scene + a shift
            self.tfs, sensor, self.map_clouds, self.origins = [], [], [], []
            for b, sc in enumerate(scenes):
                q = np.array([0.01 * (b % 3), -0.015 * (b % 2), np.sin(0.05 + 0.13 * b), np.cos(0.05 + 0.13 * b)])
                q /= np.linalg.norm(q)
                R = kitti.matrix_from_quaternion(q)
                t = np.array([sc.pos[0] + 0.7 * (b % 5) - 1.0, sc.pos[1] - 0.4 * (b % 7) + 1.0, 0.05 * (b % 3)])
                c = synth.clone_cloud(sc.cloud)
                with np.errstate(invalid="ignore", over="ignore"):  # (non-finite and huge coordinates stay what they are)
                    c["x"] = (sc.cloud["x"].astype(np.float64) - sc.pos[0]).astype(np.float32)
                    c["y"] = (sc.cloud["y"].astype(np.float64) - sc.pos[1]).astype(np.float32)
                    self.map_clouds.append(kitti.transform_cloud(c, R, t))
                sensor.append(c)
                self.tfs.append(np.hstack([R, t[:, None]]))
                self.origins.append([np.float32(v) for v in t])
            self.tfs = np.stack(self.tfs)
            self.origins = np.asarray(self.origins, np.float32)
            self.in_clouds = sensor
        else:
            self.in_clouds = [sc.cloud for sc in scenes]
            self.map_clouds = self.in_clouds
            self.origins = np.asarray([sc.origin for sc in scenes], np.float32)
        self.base_z = np.asarray([sc.base_z for sc in scenes])
        self.pts = _batch_inputs(fmt, self.in_clouds, stride)
        self.n = [len(c) for c in self.in_clouds]
        self.out = None
        hostile = {s for s, sc in enumerate(at) if sc.branch != "filler"}
        fill = sorted(set(range(n_slots)) - hostile)
        self.deep = hostile | set(fill[:: max(1, len(fill) // 6)]) | {0, n_slots - 1}

    def reset_persistent(self, slots, odom_z):
        """gg_reset_maps(persistent_only) of some slots (on the caller's stream), and the same on their oracle maps"""
        for s in slots:
            self.seg.reset_maps(first_slot=s, n_slots=1, odom_z=odom_z, pos=self.at[s].pos, persistent_only=True, on_torch_stream=True)
            r = self.refs[s]
            r.set_layer("ground", np.full((r.rows, r.cols), np.float32(odom_z)))
            r.set_layer("groundpatch", np.full((r.rows, r.cols), np.float32(0.0000001)))

    def step(self, tag, extras=False):
        import torch

        seg = self.seg
        kw = dict(slots=self.slots, transforms=self.tfs)
        if extras:  # a fresh output set that asks for every optional output
            out = seg.filter_batch(self.pts, self.n, self.origins, self.base_z, want_clouds=(self.fmt == 32), want_masks=True, want_pc2=True, **kw)
        else:
            out = self.out = seg.filter_batch(self.pts, self.n, self.origins, self.base_z, out=self.out, **kw)
        if self.halves:
            seg.batch_fence()
        torch.cuda.synchronize()
        labels, index, counts = out.labels.cpu().numpy(), out.out_index.cpu().numpy(), out.counts.cpu().numpy()
        for b, s in enumerate(self.cloud_slot):
            n, where = self.n[b], f"{tag}: cloud {b} on slot {s} ({self.at[s].name})"
            r = self.refs[s].filter_cloud(self.map_clouds[b], tuple(float(v) for v in self.origins[b]), float(self.base_z[b]))
            assert np.array_equal(labels[b, :n], r["label"]), f"{where}: {int((labels[b, :n] != r['label']).sum())} labels differ"
            assert np.array_equal(index[b, :n], r["index"]), f"{where}: emission order differs"
            emitted = r["index"] >= 0  # (the returned cloud: its kept, ignored and outlier parts)
            want = [len(r["out_points"])] + [(emitted & (r["cls"] == k)).sum() for k in (oracle.KEPT, oracle.IGNORED, oracle.OUTLIER)]
            assert counts[b].tolist() == [int(v) for v in want], f"{where}: counts {counts[b].tolist()} != {want}"
            cls, cell = seg.point_classes(n, map=seg.map(s))
            assert np.array_equal(cls, r["cls"]), f"{where}: classes differ at {np.nonzero(cls != r['cls'])[0][:5]}"
            assert np.array_equal(cell, r["cell"]), f"{where}: cells differ"
            if s not in self.deep:
                continue
            assert_same_state(seg.map(s), self.refs[s], where)
            if extras:
                k = int(counts[b, 0])
                if self.fmt == 32:
                    assert out.out_clouds[b, :k].cpu().numpy().tobytes() == r["out_points"].tobytes(), f"{where}: returned cloud"
                got = out.out_pc2[b, : k * _lib.GG_PC2_POINT_STEP].cpu().numpy().tobytes()
                assert got == api.to_pc2(r["out_points"]).tobytes(), f"{where}: PointCloud2 records"
                lab = torch.zeros((1, self.stride), dtype=torch.uint8)
                lab[0, :n] = torch.from_numpy(r["label"].copy())
                nb = (n + 3) // 4
                assert torch.equal(out.label_masks[b, :nb].cpu(), pack_label_masks(lab)[0, :nb]), f"{where}: label masks"

    def close(self):
        self.seg.synchronize()
        self.seg.close()


def _warm(run, frames, tag):
    for f in range(frames):
        run.step(f"{tag} frame {f}", extras=(f == frames - 1))


@pytest.mark.parametrize("fmt", [16, 32])
def test_case_a_24_clouds_sweep_in_parts(fmt):
    """B = 24 warm maps: more than 16 clouds, so not the pair sweep (k4_sweep.hip: launches of <= 16 clouds take it) but k_sweep cut
    into parts; k_reduce gets max(4096 / B, 64) = 170 work-groups per cloud (k2_reduce.hip); 24 slots keep the small contexts'
    chunk size.  Both point formats; hostile scenes through a slot permutation."""
    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, 24 - len(hostile), 6100)
    at, slots = _layout(24, hostile, fill, permute=True, seed=1)
    run = Run(24, at, slots, stride, fmt=fmt)
    _warm(run, 3, f"a/{fmt}")
    run.close()


def test_case_b_288_slots_2048_point_chunks():
    """A 288-slot context (>= 128 slots: 2048-point chunks in K1 / scan / scatter / K5), B = 288 (k_reduce at its floor of 64
    work-groups per cloud, the throughput k_sweep), one os128 cloud of ~260 k points among hundreds of small ones, clouds of 0, 1,
    63, 64, 65, 2047, 2048, 2049 points, stride - 1 and stride."""
    hostile = es.adversarial_scenes() + [es.sized(n, seed=1) for n in es.BATCH_SIZES]
    big = es.Scene("os128", synth.os128_cloud(seed=1, n_az=2048), "a cloud of ~260 k points")
    hostile.append(big)
    fill, stride = _with_edges_of_the_stride(hostile, 288 - len(hostile), 6200)
    at, slots = _layout(288, hostile, fill, permute=False, seed=2)
    run = Run(288, at, slots, stride)
    assert run.seg.debug_set_tuning("pw", 0) == 2048
    _warm(run, 2, "b")
    run.close()


def test_case_c_fresh_maps_then_warm_then_a_partial_cold_reset():
    """gg_reset_maps leaves fresh maps; 257 of them on 120 m satisfy sweep_takes_fresh (k4_sweep.hip), so the first launch runs
    k_patch<FRESH> and k_sweep<FRESH> on the hostile scenes; then a warm frame; then a persistent-only reset of every other pair of
    slots (a launch mixing fresh and warm maps: gg_context.hip fills the fresh ones first)."""
    B = 257
    hostile = es.adversarial_scenes() + [es.sized(n, seed=2) for n in es.BATCH_SIZES]
    fill, stride = _with_edges_of_the_stride(hostile, B - len(hostile), 6300)
    at, slots = _layout(B, hostile, fill, permute=False, seed=3)
    run = Run(B, at, slots, stride, fresh=True)
    run.step("c fresh")
    run.step("c warm")
    run.reset_persistent([s for s in range(B) if s % 4 < 2], -0.5)
    run.step("c partly cold", extras=True)
    run.close()


def test_case_d_concurrent_halves():
    """GG_FLAG_CONCURRENT_HALVES with halves_min_clouds lowered to 2 (gg_context.hip enqueue_batch: split_wanted): the clouds of the
    upper half of the slots run on the library's side stream with their own sync words; hostile clouds on both sides of the boundary
    and a slot permutation, the caller on a torch side stream, batch_fence before every read."""
    import torch

    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, 24 - len(hostile), 6400)
    at, slots = _layout(24, hostile, fill, permute=True, seed=4)
    run = Run(24, at, slots, stride, halves=True, tuning=[("halves_min_clouds", 2)])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _warm(run, 3, "d")
    side.synchronize()
    run.close()


def test_case_e_mixed_per_slot_configurations():
    """Per-slot configurations switch a launch to the SLOT_CFG kernel variants (gg_context.hip a.slot_cfg_launch): the eight
    label-tolerance configurations of test_label_tolerance_branches and the EDITS of test_slot_config_gpu.py on slots that hold
    hostile scenes (and on two that hold the label-tolerance scene's sensor cloud); the other slots follow the context."""
    hostile = es.adversarial_scenes()
    tol = es.label_tolerance(*es.LABEL_TOLERANCE_CONFIGS[0])
    hostile += [es.Scene("label_tolerance_cloud_a", tol.cloud, tol.branch, origin=tol.origin),
                es.Scene("label_tolerance_cloud_b", synth.clone_cloud(tol.cloud), tol.branch, origin=(-4.1, 6.3, 0.0))]
    fill, stride = _with_edges_of_the_stride(hostile, 26 - len(hostile), 6500)
    at, slots = _layout(26, hostile, fill, permute=True, seed=5)
    edits = [es.label_tolerance_edit(*c) for c in es.LABEL_TOLERANCE_CONFIGS] + list(EDITS)
    hostile_slots = [s for s, sc in enumerate(at) if sc.branch != "filler"]
    cfgs = {}
    for k, s in enumerate(sorted(hostile_slots, key=lambda s: (at[s].name.startswith("label_tolerance_cloud") is False, s))):
        if k < len(edits):
            cfgs[s] = make_cfg(edits[k])
    run = Run(26, at, slots, stride, slot_cfgs=cfgs)
    _warm(run, 2, "e")
    for s in cfgs:
        assert run.seg.slot_config(s)[1]
    run.close()


@pytest.mark.parametrize("knob,value", [("k2_dense_share", 4), ("sweep_waves", 1), ("sweep_waves", 3), ("front", 1), ("front", 2), ("front", 3)])
def test_case_f_launch_switches_on_case_a(knob, value):
    """Case a with one launch switch forced (gg_debug_set_tuning): k_reduce's dense / light split 4/16 instead of 12/16, one or three
    sweep wavefronts per side, the front end (classify + tile sort) as one, two or three launches."""
    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, 24 - len(hostile), 6600)
    at, slots = _layout(24, hostile, fill, permute=(value % 2 == 1), seed=6)
    run = Run(24, at, slots, stride, tuning=[(knob, value)])
    _warm(run, 2, f"f/{knob}={value}")
    run.close()


def test_case_g_distinct_transform_per_cloud():
    """B = 24 > 16 clouds in their sensor frames, each with its own map <- sensor transform fused into K1 (gg_batch.transforms): a
    cloud that read another cloud's transform, or the first one's, would land elsewhere.  The oracle is fed kitti.transform_cloud
    of each."""
    hostile = es.adversarial_scenes()
    fill, stride = _with_edges_of_the_stride(hostile, 24 - len(hostile), 6700)
    at, slots = _layout(24, hostile, fill, permute=True, seed=7)
    run = Run(24, at, slots, stride, transforms=True)
    assert len({tuple(t.ravel()) for t in run.tfs}) == 24
    _warm(run, 2, "g")
    run.close()
