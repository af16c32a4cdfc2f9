#!/usr/bin/env python
"""slot_config_step.py -- what per-map configurations (gg_set_slot_configs) cost on the headline step and on a warm fleet step.

Three modes of the same work:
  (a) none      no slot has a configuration of its own: the kernels every launch ran before
  (b) same      every slot has its own configuration EQUAL to the defaults: identical work, the SLOT_CFG kernel variants
  (c) distinct  every slot has its own configuration, all different (near the defaults): a parameter sweep of 1024 candidates
Two workloads:
  headline  bench.py's: 1024 clouds on 1024 maps of 364 x 364 (120 m / 0.33 m), fresh maps (gg_reset_maps persistent_only in every
            step), the clouds rotated over the slots by 37 per step
  fleet     tools/fleet_step.py's: warm maps that move 0.8 m per frame (gg_move_maps + gg_filter_batch over a slot permutation)
Per mode and workload: device-event-timed steps with profiling off (median / min / max of `repeats` rounds of `steps` steps after
warm-up), then one profiled round (GG_FLAG_PROFILE) for the per-kernel times.  JSON to --out, per-kernel CSV to --csv.

  python tools/slot_config_step.py [--n 1024] [--steps 10] [--repeats 5] [--out FILE] [--csv FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from groundgrid_amd import api  # noqa: E402

ROT = 37


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def distinct_configs(n):
    """n configurations near the defaults, all different (the values a parameter sweep would try)"""
    out = []
    for k in range(n):
        c = api.default_config()
        c.outlier_tolerance += 0.001 * (k % 17)
        c.distance_factor *= 1.0 + 0.01 * (k % 13)
        c.minimum_distance_factor *= 1.0 + 0.01 * (k % 11)
        c.miminum_point_height_threshold += 0.002 * (k % 7)
        c.occupied_cells_decrease_factor += 0.05 * (k % 5)
        c.ground_patch_detection_minimum_point_count_threshold *= 1.0 + 0.02 * (k % 3)
        c.patch_size_change_distance += 0.5 * ((k // 3) % 4)
        out.append(c)
    return out


def apply_mode(seg, n, mode):
    if mode == "none":
        return
    seg.set_slot_configs([api.default_config()] * n if mode == "same" else distinct_configs(n))


def run(workload, mode, n, steps, repeats, clouds):
    import torch

    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n, max_points=stride)
    apply_mode(seg, n, mode)
    host = np.zeros((n, stride), dtype=api.POINT16_DTYPE)
    npts = []
    for b in range(n):
        c = clouds[b % len(clouds)]
        host[b, : len(c)] = api.pack16(c)
        npts.append(len(c))
    pts = torch.from_numpy(host.view(np.uint8).reshape(n, stride, 16)).cuda()
    origins = np.zeros((n, 3), np.float32)
    base_z = np.full(n, -1.73)
    ids = np.arange(n)
    perm = np.random.default_rng(n).permutation(n).astype(np.int32)
    dirs = np.array([(math.cos(2.4 * k), math.sin(2.4 * k)) for k in range(n)])
    planes = np.zeros((n, 4))
    planes[:, 2], planes[:, 3] = 1.0, 1.73
    stream = torch.cuda.Stream()
    state = {"step": 0, "out": None}
    perm_p = perm.ctypes.data_as(C.POINTER(C.c_int32))
    planes_p = planes.ctypes.data_as(C.POINTER(C.c_double))
    h = C.c_void_p(stream.cuda_stream)

    def step():
        state["step"] += 1
        s = state["step"]
        if workload == "headline":
            seg.reset_maps(0, n, odom_z=0.0, persistent_only=True, on_torch_stream=True)
            slots = ((ids + ROT * s) % n).astype(np.int32)
        else:
            odom = np.ascontiguousarray(dirs * (0.8 * s))
            rc = seg._L.gg_move_maps(seg._ctx, n, perm_p, 0, odom.ctypes.data_as(C.POINTER(C.c_double)), planes_p, None, h)
            assert rc == 0, seg._L.gg_last_error(seg._ctx)
            slots = perm
        state["out"] = seg.filter_batch(pts, npts, origins, base_z, slots=slots, out=state["out"])

    torch.cuda.synchronize()
    step_ms = []
    kernels = {}
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
        for rep in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(steps):
                step()
            e1.record(stream)
            e1.synchronize()
            step_ms.append(e0.elapsed_time(e1) / steps)
        seg.set_flags(profile=True)
        step()
        seg.synchronize()
        seg.kernel_times(reset=True)
        for _ in range(steps):
            step()
        seg.synchronize()
        for name, (ms, launches) in seg.kernel_times(reset=True).items():
            kernels[name] = {"ms_per_step": ms / steps, "launches_per_step": launches / steps}
    seg.synchronize()
    r = {"workload": workload, "mode": mode, "n": n, "steps": steps, "repeats": repeats, "step_ms": stats(step_ms),
         "clouds_per_s": n * 1e3 / stats(step_ms)["median"], "kernels": kernels}
    del pts
    seg.close()
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--csv", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("slot_config_step.py measures on the GPU: none is visible")
    import bench

    clouds = bench.make_clouds(a.n, 0)
    results = []
    for workload in ("headline", "fleet"):
        for mode in ("none", "same", "distinct"):
            r = run(workload, mode, a.n, a.steps, a.repeats, clouds)
            print(json.dumps({k: r[k] for k in ("workload", "mode", "step_ms", "clouds_per_s")}), file=sys.stderr, flush=True)
            results.append(r)
    for workload in ("headline", "fleet"):
        base = next(r for r in results if r["workload"] == workload and r["mode"] == "none")
        for r in results:
            if r["workload"] != workload:
                continue
            r["step_vs_none"] = r["step_ms"]["median"] / base["step_ms"]["median"]
            for name, k in r["kernels"].items():
                b = base["kernels"][name]["ms_per_step"]
                k["vs_none"] = k["ms_per_step"] / b if b > 0 else None
    doc = {"tool": "tools/slot_config_step.py", "device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.csv)), exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("workload,mode,kernel,ms_per_step,launches_per_step,vs_none\n")
            for r in results:
                for name, k in r["kernels"].items():
                    vs = "" if k.get("vs_none") is None else f"{k['vs_none']:.4f}"
                    f.write(f"{r['workload']},{r['mode']},{name},{k['ms_per_step']:.4f},{k['launches_per_step']:.2f},{vs}\n")
    print(text)


if __name__ == "__main__":
    main()
