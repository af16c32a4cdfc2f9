#!/usr/bin/env python3
"""gg_split_clouds on the headline shape (1024 GG_POINT16 clouds on 364 x 364 maps, behind one default batch), timed by stream events,
median of --reps with the warm-up excluded, the arms alternating inside every repetition; ms per 1024 clouds:

  (a) the call, both sets with heights and sources
  (b) the call, nonground.d_points only
  (c) the floor: one device-to-device copy of as many bytes as (a) reads plus writes by the algorithmic count -- per input point 1 B of
      labels in k_split_count and 1 + 16 B in k_split_scatter, per selected point 8 B gathered and 24 B written
  (d) what callers do today: the torch loop points[b][labels[b] == 99] over --loop-clouds clouds by the wall clock (one launch sequence
      and one device -> host synchronisation per cloud), SCALED to all clouds

and the ratios (a)/(c) and (d)/(a).  Needs a GPU; writes one JSON file and prints it.

    python tools/bench_split.py --out profiles/split/summary.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--loop-clouds", type=int, default=64, help="clouds of the torch loop of arm (d)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_split.py needs a GPU")
    B = args.clouds
    base = [synth.hdl64_cloud(seed=3000 + k, n_az=args.n_az) for k in range(16)]
    stride = (max(len(c) for c in base) + 63) // 64 * 64
    host = np.zeros((16, stride), dtype=api.POINT16_DTYPE)
    for k, c in enumerate(base):
        host[k, : len(c)] = api.pack16(c)
    pts16 = torch.from_numpy(host.view(np.uint8).reshape(16, stride, 16)).cuda()
    pts = pts16.repeat((B + 15) // 16, 1, 1)[:B].contiguous()
    n_pts = [len(base[b % 16]) for b in range(B)]
    origins, base_z = np.zeros((B, 3), np.float32), np.full(B, -1.73)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        full = seg.split_clouds(pts, n_pts, labels=batch.labels)  # (the first call allocates)
        only = seg.split_clouds(pts, n_pts, labels=batch.labels, ground=False, heights=False, sources=False)
        stream.synchronize()
        counts = full.counts.cpu().numpy().astype(np.int64)
        n_in, n_sel = int(np.sum(n_pts)), int(counts.sum())
        floor_bytes = n_in * (1 + 1 + 16) + n_sel * (8 + 24)
        src = torch.empty((floor_bytes // 2,), dtype=torch.uint8, device="cuda")  # a copy of N bytes reads N / 2 and writes N / 2
        dst = torch.empty_like(src)
        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in ("a_both_sets", "b_nonground_points", "c_copy_floor"):  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "a_both_sets":
                    seg.split_clouds(pts, n_pts, labels=batch.labels, out=full)
                elif what == "b_nonground_points":
                    seg.split_clouds(pts, n_pts, labels=batch.labels, ground=False, heights=False, sources=False, out=only)
                else:
                    dst.copy_(src)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": {"clouds": B, "rows": seg.rows, "cols": seg.cols, "points_per_cloud": int(np.mean(n_pts)), "point_format": "GG_POINT16",
                         "selected_ground": int(counts[:, 0].sum()), "selected_nonground": int(counts[:, 1].sum()), "input_points": n_in},
               "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d clouds" % B, "algorithmic_bytes_of_a": floor_bytes}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    # (d) what callers do today: one boolean mask, one compaction and one synchronisation (the output size) per cloud
    n_loop = min(args.loop_clouds, B)
    recs = pts.view(B, stride, 16)

    def loop(count):
        return [recs[b, : n_pts[b]][batch.labels[b, : n_pts[b]] == 99] for b in range(count)]

    loop(min(4, n_loop))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kept = loop(n_loop)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    assert [int(k.shape[0]) for k in kept] == [int(c) for c in counts[:n_loop, 1]]
    results["d_torch_loop"] = {"clouds": n_loop, "ms_wall": wall, "ms_scaled_to_all_clouds": wall * B / n_loop, "scaled": True}
    a_ms = results["a_both_sets"]["ms_median"]
    results["ratio_a_over_c"] = a_ms / results["c_copy_floor"]["ms_median"]
    results["ratio_d_over_a"] = wall * B / n_loop / a_ms
    results["ratio_d_over_b"] = wall * B / n_loop / results["b_nonground_points"]["ms_median"]
    results["a_effective_GBps"] = floor_bytes / (a_ms * 1e-3) / 1e9
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
