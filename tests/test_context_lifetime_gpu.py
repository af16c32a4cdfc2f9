"""The lifetime of a context: everything a context allocates -- at gg_create and at the first use of an entry point -- is released by
gg_destroy, a context that failed to come up leaves nothing behind, and a context created after many others works like the first."""
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
from tests.test_export_layers_gpu import batch_points, stride_of  # noqa: E402

pytestmark = pytest.mark.gpu

ORIGIN = (0.0, 0.0, 0.0)
BASE_Z = -1.73
POSE = (0.3, 0.2, 1.5, 0.02, -0.01, 0.3, 0.95)
STATUS_OF = {v: k for k, v in _lib.STATUS.items()}


def first_use_calls(seg, cloud):
    """Once everything that allocates at its first use: move_maps and export_layers, split_clouds and cluster_clouds, set_slot_configs and
    set_score_labels, layers() of one map, filter_cloud_pc2_out, filter_cloud_with_layers with registered planes, one async ticket that is
    waited for.  Every call raises unless it returns GG_OK.  Returns the labels of the ticket's cloud."""
    import torch

    B, n = 4, len(cloud)
    stride = stride_of([cloud])
    pts = batch_points([cloud] * B, stride)
    seg.reset_maps(odom_z=0.0, on_torch_stream=True)
    out = seg.filter_batch(pts, [n] * B, np.zeros((B, 3), dtype=np.float32), [BASE_Z] * B)
    seg.move_maps([(0.4 * k, -0.3 * k) for k in range(B)], [POSE] * B, on_torch_stream=True)
    planes = seg.export_layers(n=B)
    split = seg.split_clouds(pts, [n] * B, labels=out.labels)
    clusters = seg.cluster_clouds(pts, [n] * B, labels=out.labels)
    torch.cuda.synchronize()
    assert tuple(planes.shape) == (B, len(_lib.LAYERS), seg.cols, seg.rows)
    assert int(split.counts.sum()) > 0 and int(clusters.n_clusters.min()) >= 0
    cfg = api.default_config()
    cfg.outlier_tolerance = 0.2
    seg.set_slot_configs([cfg], slots=[1])
    seg.set_score_labels()
    layers = seg.map(0).layers()
    assert set(layers) == set(_lib.LAYERS)
    pc2 = api.to_pc2(cloud)
    returned = seg.filter_cloud_pc2_out(pc2.tobytes(), n, 18, (0, 4, 8, 16), ORIGIN, BASE_Z, map=seg.map(2))
    assert 0 < len(returned) <= n
    host_planes = seg.alloc_layers(["ground", "points", "variance"], register=True)
    seg.filter_cloud_with_layers(cloud, ORIGIN, BASE_Z, host_planes, map=seg.map(3))
    seg.release_layers(host_planes)
    assert np.array_equal(host_planes["ground"], seg.map(3).get("ground"))
    seg.map(0).reset(0.0)
    ticket = seg.filter_cloud_async(cloud, ORIGIN, BASE_Z)
    _, labels, _ = seg.filter_cloud_wait(ticket, return_details=True)
    return labels.copy()


def test_every_first_use_path_then_destroy():
    cloud = synth.hdl64_cloud(seed=9100, n_az=60)[:4096]
    labels = []
    for _ in range(4):
        seg = api.GroundSegmentation().init(20.0, 0.33, n_slots=4, max_points=4096)
        labels.append(first_use_calls(seg, cloud))
        seg.close()
    assert len(labels[0]) == len(cloud)
    assert np.array_equal(labels[3], labels[0])


def test_no_leak_across_cycles():
    """Eight create / use / close cycles of a 64-slot context do not lose device memory: free memory after the eighth is not below free
    memory after the first by more than half a context's footprint.  A leaked arena would show as seven footprints.  A leaked small block
    (a first-use scratch, a staging block) is what the owner types of csrc/hip_owned.h rule out by construction; this test cannot see one."""
    import torch

    cloud = synth.hdl64_cloud(seed=9200, n_az=60)[:4096]
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    free_after = []
    footprint = None
    for cycle in range(8):
        seg = api.GroundSegmentation().init(40.0, 0.33, n_slots=64, max_points=32768)
        if cycle == 0:
            footprint = free_before - torch.cuda.mem_get_info()[0]
        first_use_calls(seg, cloud)
        seg.close()
        torch.cuda.synchronize()
        free_after.append(torch.cuda.mem_get_info()[0])
    print(f"footprint {footprint} B, free before {free_before} B, free after each cycle {free_after}")
    assert footprint > 64 << 20  # (64 slots of 32768 points: the arena alone is larger)
    assert free_after[7] >= free_after[0] - footprint // 2


def create_status(length, resolution, n_slots=1, max_points=4096):
    L = _lib.load()
    geom = _lib.GGGeometry(float(length), float(resolution), 0.0, 0.0)
    ctx = C.c_void_p()
    rc = L.gg_create(C.byref(geom), n_slots, max_points, 0, C.byref(ctx))
    assert (rc == _lib.GG_OK) == bool(ctx.value)
    if ctx.value:
        L.gg_destroy(ctx)
    return rc


def test_a_failed_create_leaves_nothing_behind(monkeypatch):
    """Error returns only: GG_PW=100 (no multiple of 64) is rejected after the streams and events exist; a map of length 3 at resolution
    0.5 has 6 x 6 cells, below gg_create's minimum of 8, and is rejected before anything does."""
    monkeypatch.setenv("GG_PW", "100")
    for _ in range(4):
        assert create_status(20.0, 0.33) == STATUS_OF["GG_ERR_INVALID"]
    monkeypatch.delenv("GG_PW")
    assert create_status(3.0, 0.5) == STATUS_OF["GG_ERR_GEOMETRY"]
    cloud = synth.hdl64_cloud(seed=9300, n_az=60)[:4096]
    seg = api.GroundSegmentation().init(20.0, 0.33, n_slots=1, max_points=4096)
    ref = oracle.OracleMap(20.0, 0.33)
    _, labels, index = seg.filter_cloud(cloud, ORIGIN, BASE_Z, return_details=True)
    r = ref.filter_cloud(cloud, ORIGIN, BASE_Z)
    assert np.array_equal(labels, r["label"]) and np.array_equal(index, r["index"])
    assert np.array_equal(seg.map(0).get("ground"), ref.layer("ground"))
    seg.close()
