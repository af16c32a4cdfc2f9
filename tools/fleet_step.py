#!/usr/bin/env python
"""fleet_step.py -- what it costs to scroll N moving maps to their odometry, one map per call against one call for all, and a whole
fleet step (gg_move_maps + gg_filter_batch over the same slots).

For every N (maps of 364 x 364 = 120 m / 0.33 m; 1000 x 1000 = 200 m / 0.2 m at N <= 64), each vehicle drives 0.8 m per frame in
its own direction, so every map scrolls by two or three cells every frame (warm maps that move, the fleet-server case):
  (a) per_slot   N gg_move_map calls (the context's stream)                       ms per frame
  (b) move_maps  one gg_move_maps call for the N maps (the context's stream)       ms per frame
  (c) fleet      gg_move_maps + gg_filter_batch(slots) on one torch stream         ms per frame and clouds/s
(a) and (b) are timed by the host clock around `frames` calls that end in gg_synchronize, (c) by device events around `frames`
steps; all after warm-up, `repeats` times (median, min, max).  The ctypes arguments are prepared before the timed region, so (a)
and (b) measure the library's calls, not the Python binding.  One JSON document goes to --out (and stdout).

  python tools/fleet_step.py [--n 1 16 64 256 1024] [--frames 10] [--repeats 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from groundgrid_amd import api, synth  # noqa: E402

GRIDS = {364: (120.0, 0.33), 1000: (200.0, 0.2)}
STEP_M = 0.8


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


class Fleet:
    """N vehicles: vehicle k heads at angle 2.4 k rad; frame f puts it at f * 0.8 m along that heading."""

    def __init__(self, n):
        self.n = n
        self.dirs = np.array([(math.cos(2.4 * k), math.sin(2.4 * k)) for k in range(n)])

    def frame(self, f):
        odom = np.ascontiguousarray(self.dirs * (STEP_M * f))
        planes = np.zeros((self.n, 4))
        planes[:, 2] = 1.0
        planes[:, 3] = 1.73
        return odom, planes


def measure(grid, n, frames, repeats, clouds):
    import torch

    length, res = GRIDS[grid]
    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(length, res, n_slots=n, max_points=stride)
    L, ctx = seg._L, seg._ctx
    fleet = Fleet(n)
    slots = np.ascontiguousarray(np.random.default_rng(n).permutation(n).astype(np.int32))
    P = C.POINTER
    frame_no = [0]

    def prepared(count):  # the next `count` frames' arguments, ready for the calls
        out = []
        for _ in range(count):
            frame_no[0] += 1
            odom, planes = fleet.frame(frame_no[0])
            out.append((odom, planes, odom.ctypes.data_as(P(C.c_double)), planes.ctypes.data_as(P(C.c_double))))
        return out

    slot_list = [int(s) for s in slots]
    plane = (C.c_double * 4)(0.0, 0.0, 1.0, 1.73)  # (every vehicle's Fleet.frame plane)

    def per_slot(args):
        for odom, _, _, _ in args:
            ox, oy = odom[:, 0].tolist(), odom[:, 1].tolist()
            for k in range(n):
                rc = L.gg_move_map(ctx, slot_list[k], ox[k], oy[k], plane, None)
                assert rc == 0, rc

    sl = slots.ctypes.data_as(P(C.c_int32))

    def batched(args, stream=None):
        for _, _, po, pp in args:
            rc = L.gg_move_maps(ctx, n, sl, 0, po, pp, None, stream)
            assert rc == 0, L.gg_last_error(ctx)

    def timed_host(fn):
        out = []
        for _ in range(repeats):
            args = prepared(frames)
            seg.synchronize()
            t0 = time.perf_counter()
            fn(args)
            seg.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / frames)
        return stats(out)

    per_slot(prepared(2))
    batched(prepared(2))
    seg.synchronize()
    res_a = timed_host(per_slot)
    res_b = timed_host(batched)

    # (c) the fleet step on one torch stream
    B = n
    host = np.zeros((B, stride), dtype=api.POINT16_DTYPE)
    npts = []
    for b in range(B):
        c = clouds[b % len(clouds)]
        host[b, : len(c)] = api.pack16(c)
        npts.append(len(c))
    pts = torch.from_numpy(host.view(np.uint8).reshape(B, stride, 16)).cuda()
    origins = np.zeros((B, 3), np.float32)
    base_z = np.full(B, -1.73)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    h = C.c_void_p(stream.cuda_stream)
    out = None
    res_c = []
    with torch.cuda.stream(stream):
        for rep in range(repeats + 1):
            args = prepared(frames)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for a in args:
                batched([a], h)
                out = seg.filter_batch(pts, npts, origins, base_z, slots=slots.tolist(), out=out)
            e1.record(stream)
            e1.synchronize()
            if rep:  # (the first round warms up)
                res_c.append(e0.elapsed_time(e1) / frames)
    seg.synchronize()
    fleet_ms = stats(res_c)
    cells = grid * grid
    r = {"grid": grid, "n_maps": n, "frames": frames, "repeats": repeats,
         "per_slot_move_ms": res_a, "move_maps_ms": res_b,
         "fleet_step_ms": fleet_ms, "fleet_clouds_per_s": {"median": B * 1e3 / fleet_ms["median"], "min": B * 1e3 / fleet_ms["max"], "max": B * 1e3 / fleet_ms["min"]},
         "points_per_cloud_mean": float(np.mean(npts)),
         "scroll_bytes_per_frame": 4 * cells * 8 * n}  # algorithmic: read old cells, write + read scratch, write new cells (8 B a cell)
    r["move_maps_speedup"] = res_a["median"] / res_b["median"]
    del pts, out
    seg.close()
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--big-max", type=int, default=64, help="1000 x 1000 maps for N up to this")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("fleet_step.py measures on the GPU: none is visible")
    clouds = [synth.hdl64_cloud(seed=20240113 + k) for k in range(a.scenes)]
    results = []
    for grid in (364, 1000):
        for n in a.n:
            if grid == 1000 and n > a.big_max:
                continue
            r = measure(grid, n, a.frames, a.repeats, clouds)
            print(json.dumps(r), file=sys.stderr, flush=True)
            results.append(r)
    doc = {"tool": "tools/fleet_step.py", "device": torch.cuda.get_device_name(0), "step_m": STEP_M, "results": results}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
