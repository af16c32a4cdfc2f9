"""The HIP path against the recorded results of the reference build (pytest -m gpu, on a real MI355X), without the oracle in between.

tests/golden/ref_build_digests.json holds, per scene and frame, digests of what the reference's own translation unit -- compiled
against stand-ins, oracle/ref_build.py -- returned and left in the map (written by oracle/ref_record.py from that binary alone).
Here gg_filter_cloud + gg_get_layers, and one batched launch holding all 364-cell scenes at once, reproduce those digests directly:
the returned cloud by its bytes (labels 49 / 99, order), all 11 layers by their bits (NaN == NaN, -0.0 != 0.0).  Only tests/golden/
and the seeded generators are read: the reference does not exist on the GPU machine.  The line-of-sight walk is bounded on the
device (documented deviation), which is why the one scene the digests exclude is excluded: see tests/ref_scenes.py EXCLUDED.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from groundgrid_amd import api  # noqa: E402
from tests import geom_sets as gs  # noqa: E402
from tests import ref_scenes as rs  # noqa: E402


def _check_frame(name, f, rec, out_bytes, layers):
    got = rs.frame_digest(out_bytes, layers)
    want = rec["frames"][f]
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{name} frame {f}: the device does not reproduce the reference build's {bad} (n = {got['n']}, recorded {want['n']})"


def _recorded(name, scene):
    rec = rs.load_digests()["scenes"][name]
    assert rs.input_digest(scene) == rec["input"], f"{name}: the scene generator drifted from the inputs the digests were recorded from"
    return rec


@pytest.mark.parametrize("name", rs.names())
def test_single_cloud_calls_reproduce_the_reference_digests(name):
    scene = rs.scene(name)
    rec = _recorded(name, scene)
    vpad, mds = gs.scene_constants(scene)   # (the geom/ scenes: the pair their reference binary was compiled with)
    seg = api.GroundSegmentation().init(scene.length, scene.resolution, n_slots=1, max_points=max(len(scene.cloud), 1),
                                        vertical_point_ang_dist=vpad, min_dist_squared=mds)
    seg.map(0).reset(odom_z=scene.odom_z, pos=scene.pos)
    if scene.cfg_edit:
        c = seg.getConfig()
        scene.cfg_edit(c)
        seg.setConfig(c)
    for f in range(scene.frames):
        out = seg.filter_cloud(gs.frame_cloud(scene, f), scene.origin, scene.base_z)
        _check_frame(name, f, rec, rs.cloud_bytes(out), seg.map(0).layers())
    seg.close()


def test_one_batched_launch_of_every_364_cell_scene_reproduces_the_reference_digests():
    """all scenes on the 120 m / 0.33 m grid in ONE gg_filter_batch per frame: every slot its own map position, initial height and
    configuration; scenes with fewer frames repeat their last cloud on a slot whose digests are no longer checked"""
    import torch

    names = [n for n in rs.names() if (np.float32(rs.scene(n).length), np.float32(rs.scene(n).resolution)) == (np.float32(120.0), np.float32(0.33))
             and "variant" not in rs.scene(n).extra]   # (a context has one pair of sensor constants: the geom/ scenes run in the test above)
    assert len(names) >= 45
    scenes = [rs.scene(n) for n in names]
    recs = [_recorded(n, s) for n, s in zip(names, scenes)]
    B = len(scenes)
    stride = (max(len(s.cloud) for s in scenes) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    own = {}
    for b, s in enumerate(scenes):
        if s.pos != (0.0, 0.0) or s.odom_z != 0.0:
            seg.map(b).reset(odom_z=s.odom_z, pos=s.pos)
        if s.cfg_edit:
            own[b] = api.default_config()
            s.cfg_edit(own[b])
    seg.set_slot_configs([own[b] for b in sorted(own)], slots=sorted(own))
    raw = np.zeros((B, stride, 32), dtype=np.uint8)
    for b, s in enumerate(scenes):
        raw[b, : len(s.cloud)] = rs.cloud_bytes(s.cloud)
    pts = torch.from_numpy(raw).cuda()
    origins = np.asarray([s.origin for s in scenes], np.float32)
    base_z = np.asarray([s.base_z for s in scenes])
    n = [len(s.cloud) for s in scenes]
    for f in range(max(s.frames for s in scenes)):
        out = seg.filter_batch(pts, n, origins, base_z, want_clouds=True)
        torch.cuda.synchronize()
        clouds, index = out.out_clouds.cpu().numpy(), out.out_index.cpu().numpy()
        for b, s in enumerate(scenes):
            if f < s.frames:
                n_out = int((index[b, : n[b]] >= 0).sum())
                _check_frame(f"batched {names[b]}", f, recs[b], clouds[b, :n_out], seg.map(b).layers())
    seg.close()
