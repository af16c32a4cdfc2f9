#!/usr/bin/env python3
"""gg_rasterize_clouds on the headline shape (1024 GG_POINT16 clouds on 364 x 364 maps, behind one default batch), timed by stream events,
median of --reps with the warm-up excluded, the arms alternating inside every repetition; ms per 1024 clouds:

  (a) the call with the two default channels (non-ground count and max height)
  (b) the call with all six channels
  (c) the floor: one device-to-device copy of as many bytes as (a) reads plus writes by the algorithmic count -- per input point 1 + 16 B,
      per non-ground point inside its map 8 B gathered and 2 x 4 B of atomics, per cell and plane 4 B written by the first launch and
      4 + 4 B read and written by the third
  (d) what callers do today for the same two planes: split_clouds (non-ground records and heights), then torch: the cell of every record
      from the map position and the grid_map index arithmetic restated in float64, index_add_ for the count and scatter_reduce_(amax) for
      the height, over the whole batch at once

and the ratios (a)/(c) and (d)/(a).  (d)'s planes are compared with (a)'s before anything is timed.  Needs a GPU; writes one JSON file
and prints it.

    python tools/bench_raster.py --out profiles/raster/summary.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_raster.py needs a GPU")
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
    rows, cols, cells = seg.rows, seg.cols, seg.rows * seg.cols
    res = float(np.float32(0.33))
    size_m = rows * res  # grid_map's length: size * resolution
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        two = seg.rasterize_clouds(pts, n_pts, labels=batch.labels)  # (the first call allocates)
        six = seg.rasterize_clouds(pts, n_pts, labels=batch.labels, channels=_lib.RASTER_CHANNELS)
        split = seg.split_clouds(pts, n_pts, labels=batch.labels, ground=False, sources=False)
        count_d = torch.empty((B * cells,), dtype=torch.float32, device="cuda")
        high_d = torch.empty((B * cells,), dtype=torch.float32, device="cuda")
        slot_of = torch.arange(B, device="cuda").view(B, 1)
        lane = torch.arange(stride, device="cuda").view(1, stride)
        ones = torch.ones((B * stride,), dtype=torch.float32, device="cuda")

        def torch_arm():
            """what a caller writes today (every map sits at position (0, 0) here; a caller has to carry the positions along)"""
            seg.split_clouds(pts, n_pts, labels=batch.labels, ground=False, sources=False, out=split)
            xyz = split.nonground_points.view(torch.float32).view(B, stride, 4)
            r = (-((xyz[:, :, 0].double() - 0.5 * size_m) / res)).to(torch.int64)
            c = (-((xyz[:, :, 1].double() - 0.5 * size_m) / res)).to(torch.int64)
            ok = (lane < split.counts[:, 1:2]) & (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
            idx = torch.where(ok, slot_of * cells + r * cols + c, torch.zeros_like(r)).view(-1)
            w = ok.view(-1)
            count_d.zero_()
            count_d.index_add_(0, idx, ones * w)
            high_d.fill_(float("-inf"))
            high_d.scatter_reduce_(0, idx, torch.where(w, split.nonground_height.view(-1), torch.full_like(ones, float("-inf"))), "amax", include_self=True)
            high_d.masked_fill_(high_d == float("-inf"), float("nan"))

        torch_arm()
        stream.synchronize()
        n_in = int(np.sum(n_pts))
        n_sel = int(two[:, 0].sum().item())
        same_count = bool(torch.equal(count_d.view(B, rows, cols), two[:, 0]))
        same_high = bool(torch.equal(high_d.view(B, rows, cols).view(torch.int32), two[:, 1].view(torch.int32)))
        floor_bytes = n_in * (1 + 16) + n_sel * (8 + 2 * 4) + B * cells * 2 * (4 + 4 + 4)
        src = torch.empty((floor_bytes // 2,), dtype=torch.uint8, device="cuda")  # a copy of N bytes reads N / 2 and writes N / 2
        dst = torch.empty_like(src)
        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in ("a_two_channels", "b_six_channels", "c_copy_floor", "d_split_and_torch"):  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "a_two_channels":
                    seg.rasterize_clouds(pts, n_pts, labels=batch.labels, out=two)
                elif what == "b_six_channels":
                    seg.rasterize_clouds(pts, n_pts, labels=batch.labels, channels=_lib.RASTER_CHANNELS, out=six)
                elif what == "c_copy_floor":
                    dst.copy_(src)
                else:
                    torch_arm()
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": {"clouds": B, "rows": rows, "cols": cols, "points_per_cloud": int(np.mean(n_pts)), "point_format": "GG_POINT16",
                         "input_points": n_in, "nonground_points_inside": n_sel},
               "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d clouds" % B, "algorithmic_bytes_of_a": floor_bytes,
               "d_equals_a": {"count": same_count, "max_height": same_high}}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    a_ms = results["a_two_channels"]["ms_median"]
    results["ratio_a_over_c"] = a_ms / results["c_copy_floor"]["ms_median"]
    results["ratio_d_over_a"] = results["d_split_and_torch"]["ms_median"] / a_ms
    results["ratio_b_over_a"] = results["b_six_channels"]["ms_median"] / a_ms
    results["a_effective_GBps"] = floor_bytes / (a_ms * 1e-3) / 1e9
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
