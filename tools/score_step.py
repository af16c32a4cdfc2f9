#!/usr/bin/env python
"""score_step.py -- what the evaluator counters (gg_set_slot_scoring, k8_score.hip) cost on the headline step, and what they replace.

bench.py's workload: 1024 clouds on 1024 maps of 364 x 364 (120 m / 0.33 m), fresh maps (gg_reset_maps persistent_only in every step),
the clouds rotated over the slots by 37 per step.  Three modes:
  (a) none   no slot scores: the kernels every launch ran before
  (b) all    every slot scores: k_score behind k_label, the counters stay on the device
  (c) host   today's alternative: (a), then d_labels and d_out_index come down and GroundEvaluator.add_cloud runs per cloud on the host
             (host clock around step + download + loop: it is host work)
(a) and (b): device-event-timed steps with profiling off (median / min / max of `repeats` rounds of `steps` steps after warm-up), then
one profiled round (GG_FLAG_PROFILE) for the per-kernel times -- k_score next to k_classify, which streams the same point bytes.
JSON to --out, per-kernel CSV to --csv.

  python tools/score_step.py [--n 1024] [--steps 10] [--repeats 5] [--host-steps 1] [--out FILE] [--csv FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from groundgrid_amd import api  # noqa: E402
from groundgrid_amd.evaluate import GroundEvaluator  # noqa: E402

ROT = 37


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def run(mode, n, steps, repeats, host_steps, clouds):
    import torch

    stride = (max(len(c) for c in clouds) + 63) // 64 * 64
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=n, max_points=stride)
    if mode == "all":
        seg.set_scoring()
    host = np.zeros((n, stride), dtype=api.POINT16_DTYPE)
    npts, rings = [], []
    for b in range(n):
        c = clouds[b % len(clouds)]
        host[b, : len(c)] = api.pack16(c)
        npts.append(len(c))
        rings.append(c["ring"])
    pts = torch.from_numpy(host.view(np.uint8).reshape(n, stride, 16)).cuda()
    origins = np.zeros((n, 3), np.float32)
    base_z = np.full(n, -1.73)
    ids = np.arange(n)
    stream = torch.cuda.Stream()
    state = {"step": 0, "out": None}

    def step():
        state["step"] += 1
        seg.reset_maps(0, n, odom_z=0.0, persistent_only=True, on_torch_stream=True)
        slots = ((ids + ROT * state["step"]) % n).astype(np.int32)
        state["out"] = seg.filter_batch(pts, npts, origins, base_z, slots=slots, out=state["out"])
        return slots

    torch.cuda.synchronize()
    r = {"mode": mode, "n": n, "points_per_step": int(sum(npts))}
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
        if mode == "host":
            evs = [GroundEvaluator() for _ in range(n)]
            t = []
            for _ in range(host_steps):
                stream.synchronize()
                t0 = time.perf_counter()
                slots = step()
                labels = state["out"].labels.cpu().numpy()
                index = state["out"].out_index.cpu().numpy()
                t1 = time.perf_counter()
                for b in range(n):
                    m = npts[b]
                    emitted = index[b, :m] >= 0
                    evs[int(slots[b])].add_cloud(labels[b, :m][emitted], rings[b][emitted], allow_unknown=True)
                t2 = time.perf_counter()
                t.append({"step_ms": 1e3 * (t2 - t0), "step_and_download_ms": 1e3 * (t1 - t0), "add_cloud_loop_ms": 1e3 * (t2 - t1)})
            r["host_steps"] = t
            r["step_ms"] = stats([x["step_ms"] for x in t])
            r["download_bytes_per_step"] = int(n * stride * 5)
        else:
            step_ms = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(steps):
                    step()
                e1.record(stream)
                e1.synchronize()
                step_ms.append(e0.elapsed_time(e1) / steps)
            r["step_ms"] = stats(step_ms)
            seg.set_flags(profile=True)
            step()
            seg.synchronize()
            seg.kernel_times(reset=True)
            seg.score_kernel_time(reset=True)
            for _ in range(steps):
                step()
            seg.synchronize()
            kernels = {}
            for name, (ms, launches) in seg.kernel_times(reset=True).items():
                kernels[name] = {"ms_per_step": ms / steps, "launches_per_step": launches / steps}
            ms, launches = seg.score_kernel_time(reset=True)
            kernels["k_score"] = {"ms_per_step": ms / steps, "launches_per_step": launches / steps}
            r["kernels"] = kernels
            if mode == "all":
                clouds_scored, counts = seg.scores_raw()
                r["clouds_scored_per_slot"] = [int(clouds_scored.min()), int(clouds_scored.max())]
                r["points_counted"] = int(counts.sum())
                # the bytes the pass needs: the 16-byte record and a quarter byte of label mask per point
                b = r["points_per_step"] * 16.25
                r["k_score_algorithmic_gb_per_s"] = b / (kernels["k_score"]["ms_per_step"] * 1e6) if kernels["k_score"]["ms_per_step"] > 0 else None
                r["k_classify_algorithmic_gb_per_s"] = r["points_per_step"] * 16.0 / (kernels["k_classify"]["ms_per_step"] * 1e6)
    seg.synchronize()
    r["clouds_per_s"] = n * 1e3 / r["step_ms"]["median"]
    del pts
    seg.close()
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=1)
    ap.add_argument("--out", default="")
    ap.add_argument("--csv", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("score_step.py measures on the GPU: none is visible")
    import bench

    clouds = bench.make_clouds(a.n, 0)
    results = []
    for mode in ("none", "all", "none", "all", "host"):  # (a) and (b) twice, alternating: the spread of the box is in the record
        r = run(mode, a.n, a.steps, a.repeats, a.host_steps, clouds)
        print(json.dumps({k: r[k] for k in ("mode", "step_ms", "clouds_per_s")}), file=sys.stderr, flush=True)
        results.append(r)
    doc = {"tool": "tools/score_step.py", "device": torch.cuda.get_device_name(0), "results": results}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.csv:
        os.makedirs(os.path.dirname(os.path.abspath(a.csv)), exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("run,mode,kernel,ms_per_step,launches_per_step\n")
            for k, r in enumerate(results):
                for name, v in r.get("kernels", {}).items():
                    f.write(f"{k},{r['mode']},{name},{v['ms_per_step']:.4f},{v['launches_per_step']:.2f}\n")
    print(text)


if __name__ == "__main__":
    main()
