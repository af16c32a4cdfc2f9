"""Host cost of a device call: 2000 back-to-back enqueues, one synchronisation at the end, wall time per call.
usage: python tools/plane_call_cost.py PACKAGE_ROOT LABEL OUT_DIR [CALL ...]   (PACKAGE_ROOT: the directory that holds the groundgrid_amd package to
time, its built library in it: the repository root, or a copy of another commit's package for an A/B in one session.  CALL: the names of
TIMED below; default: the two plane calls)"""
import ctypes as C
import json
import os
import sys
import time

pkg_root, label, out_dir = sys.argv[1:4]
names = sys.argv[4:] or ["gg_fuse_states_raw", "route_planes_out"]
sys.path.insert(0, os.path.abspath(pkg_root))
import torch  # noqa: E402
from groundgrid_amd import _lib, api  # noqa: E402

assert os.path.abspath(api.__file__).startswith(os.path.abspath(pkg_root)), api.__file__
CALLS, WARM, REPEATS = 2000, 200, 3
seg = api.GroundSegmentation().init(7.0, 0.35, n_slots=4, max_points=4096)
assert seg.rows == seg.cols == 20
cells = 400
z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
L, ctx = seg._L, seg._ctx


def raw(call, x):
    def run(k):
        for _ in range(k):
            rc = call(ctx, C.byref(x), None)
            assert rc == 0, rc
    return run


def method(call, **kw):
    """a method with the `out` its first call returned"""
    out = call(**kw)

    def run(k):
        for _ in range(k):
            call(out=out, **kw)
    return run


def fuse():
    state, ev_in, ev_out, fused, frontier, counts = z(1, 20, 20), z(1, 20, 20), z(1, 20, 20), z(1, 20, 20), z(1, 20, 20), z(1, 4)
    x = _lib.GGStateFusion()
    x.n, x.d_state, x.state_stride, x.d_evidence_in = 1, state.data_ptr(), cells, ev_in.data_ptr()
    x.hit, x.miss, x.decay, x.e_min, x.e_max, x.free_threshold, x.occ_threshold = 4, 1, 0, -16, 32, -2, 4
    x.order, x.d_evidence_out, x.plane_stride = _lib.GG_PLANES_ROWMAJOR, ev_out.data_ptr(), cells
    x.d_fused, x.d_frontier, x.d_counts = fused.data_ptr(), frontier.data_ptr(), counts.data_ptr()
    return raw(L.gg_fuse_states, x), (state, ev_in, ev_out, fused, frontier, counts)


# the labelled clouds of tests/cloud_refusals.py with n = 1: 40 zero-filled POINT16 points, cloud_stride = 64, labels given
points, labels, n_points = z(1, 64, 16, dtype=torch.uint8), z(1, 64, dtype=torch.uint8), (C.c_int32 * 1)(40)


def rasterize():
    dst = z(1, len(_lib.RASTER_CHANNELS), 20, 20, dtype=torch.float32)
    x = _lib.GGCloudRaster()
    x.n, x.point_format, x.d_points, x.cloud_stride, x.n_points, x.d_labels = 1, _lib.GG_POINT16, points.data_ptr(), 64, n_points, labels.data_ptr()
    x.channel_mask, x.order, x.d_dst, x.plane_stride = (1 << len(_lib.RASTER_CHANNELS)) - 1, _lib.GG_PLANES_ROWMAJOR, dst.data_ptr(), cells
    return raw(L.gg_rasterize_clouds, x), dst


TIMED = {"gg_fuse_states_raw": fuse, "route_planes_out": lambda: (method(seg.route_planes, goals=z(1, 20, 20)), None),
         "gg_rasterize_clouds_raw": rasterize, "cluster_clouds_out": lambda: (method(seg.cluster_clouds, points=points, n_points=[40], labels=labels), None),
         "export_layers_out": lambda: (method(seg.export_layers, n=1), None)}


def timed(fn):
    fn(WARM)
    torch.cuda.synchronize()
    runs = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn(CALLS)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / CALLS * 1e6)
    return runs


res = {"label": label, "calls": CALLS, "map": "20 x 20, n = 1", "unit": "microseconds per call, wall, one synchronisation behind the last call"}
for name in names:
    run, keep = TIMED[name]()   # (keep: the device buffers a raw call points to)
    res[name] = timed(run)
seg.close()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{label}.json"), "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
