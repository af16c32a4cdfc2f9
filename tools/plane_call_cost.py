"""Host cost of a plane call: 2000 back-to-back enqueues, one synchronisation at the end, wall time per call.
usage: python tools/plane_call_cost.py PACKAGE_ROOT LABEL OUT_DIR   (PACKAGE_ROOT: the directory that holds the groundgrid_amd package to time,
its built library in it: the repository root, or a copy of another commit's package for an A/B in one session)"""
import ctypes as C
import json
import os
import sys
import time

pkg_root, label, out_dir = sys.argv[1:4]
sys.path.insert(0, os.path.abspath(pkg_root))
import torch  # noqa: E402
from groundgrid_amd import _lib, api  # noqa: E402

assert os.path.abspath(api.__file__).startswith(os.path.abspath(pkg_root)), api.__file__
CALLS, WARM, REPEATS = 2000, 200, 3
seg = api.GroundSegmentation().init(7.0, 0.35, n_slots=4, max_points=4096)
assert seg.rows == seg.cols == 20
cells = 400
z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
state, ev_in, ev_out, fused, frontier, counts = z(1, 20, 20), z(1, 20, 20), z(1, 20, 20), z(1, 20, 20), z(1, 20, 20), z(1, 4)
x = _lib.GGStateFusion()
x.n, x.d_state, x.state_stride, x.d_evidence_in = 1, state.data_ptr(), cells, ev_in.data_ptr()
x.hit, x.miss, x.decay, x.e_min, x.e_max, x.free_threshold, x.occ_threshold = 4, 1, 0, -16, 32, -2, 4
x.order, x.d_evidence_out, x.plane_stride = _lib.GG_PLANES_ROWMAJOR, ev_out.data_ptr(), cells
x.d_fused, x.d_frontier, x.d_counts = fused.data_ptr(), frontier.data_ptr(), counts.data_ptr()
L, ctx = seg._L, seg._ctx


def fuse(k):
    for _ in range(k):
        rc = L.gg_fuse_states(ctx, C.byref(x), None)
        assert rc == 0, rc


goals = z(1, 20, 20)
out = seg.route_planes(goals)


def route(k):
    for _ in range(k):
        seg.route_planes(goals, out=out)


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


res = {"label": label, "calls": CALLS, "map": "20 x 20, n = 1", "unit": "microseconds per call, wall, one synchronisation behind the last call",
       "gg_fuse_states_raw": timed(fuse), "route_planes_out": timed(route)}
seg.close()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{label}.json"), "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
