#!/usr/bin/env python3
"""gg_cluster_clouds on the headline shape of tools/bench_raster.py (1024 GG_POINT16 clouds of a 64-ring scan on 364 x 364 maps, labels
from one default batch), timed by stream events, median of --reps with the warm-up excluded, the arms alternating inside every repetition;
ms per 1024 clouds:

  conn8_all / conn4_all      the call with the table (max_clusters 256) and the per-point ids, open band, min_points 1
  conn8_plane / conn4_plane  the id plane and the counts alone (max_clusters 0, no per-point ids: no second pass over the points)
  conn8_band                 conn8_all with min_points 2 and the band [0.3, 2.5] (the ground is gathered in both point passes)
  raster_count               gg_rasterize_clouds(nonground_count) alone, for scale

and what a caller does today for the same id planes, timed by the wall clock on --host-maps maps and scaled to the 1024: rasterize_clouds
(nonground_count), the planes to the host, scipy.ndimage.label per map, the label planes back to the device.  Its planes are compared with
conn8_plane's before anything is timed.  Needs a GPU; writes one JSON file and prints it.  For times per kernel run the tool alone under
`rocprofv3 --kernel-trace --stats -- python tools/bench_cluster.py --reps 3`.

    python tools/bench_cluster.py --out profiles/cluster/summary.json
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
    ap.add_argument("--host-maps", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_cluster.py needs a GPU")
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
    rows, cols = seg.rows, seg.cols
    arms = {"conn8_all": dict(connectivity=8), "conn4_all": dict(connectivity=4),
            "conn8_plane": dict(connectivity=8, max_clusters=0, point_clusters=False), "conn4_plane": dict(connectivity=4, max_clusters=0, point_clusters=False),
            "conn8_band": dict(connectivity=8, min_points=2, min_height=0.3, max_height=2.5)}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        outs = {name: seg.cluster_clouds(pts, n_pts, labels=batch.labels, **kw) for name, kw in arms.items()}  # (the first call allocates)
        count = seg.rasterize_clouds(pts, n_pts, labels=batch.labels, channels=["nonground_count"])
        stream.synchronize()
        K8, K4 = outs["conn8_all"].n_clusters.cpu().numpy(), outs["conn4_all"].n_clusters.cpu().numpy()
        occupied = int((count > 0).sum().item())

        # what a caller does today, on the first host-maps maps
        H = min(args.host_maps, B)
        host_result = None
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None and H > 0:
            full = np.ones((3, 3), dtype=np.int32)

            def host_arm():
                planes = seg.rasterize_clouds(pts[:H], n_pts[:H], labels=batch.labels[:H], channels=["nonground_count"])
                grid = planes[:, 0].cpu().numpy()
                lab = np.stack([ndimage.label(grid[b] > 0, structure=full)[0] for b in range(H)]).astype(np.int32) - 1
                return torch.from_numpy(lab).cuda()

            same = bool(torch.equal(host_arm(), outs["conn8_plane"].cell_cluster[:H]))
            walls = []
            for _ in range(args.host_reps):
                stream.synchronize()
                t0 = time.perf_counter()
                host_arm()
                stream.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
            host_result = {"maps": H, "ms_median_measured": float(np.median(walls)), "ms_scaled_to_all_clouds": float(np.median(walls)) * B / H,
                           "equals_conn8_plane": same}

        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in list(arms) + ["raster_count"]:  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "raster_count":
                    seg.rasterize_clouds(pts, n_pts, labels=batch.labels, channels=["nonground_count"], out=count)
                else:
                    seg.cluster_clouds(pts, n_pts, labels=batch.labels, out=outs[what], **arms[what])
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": {"clouds": B, "rows": rows, "cols": cols, "points_per_cloud": int(np.mean(n_pts)), "point_format": "GG_POINT16",
                         "input_points": int(np.sum(n_pts)), "occupied_cells": occupied, "clusters_per_map_conn8": float(K8.mean()),
                         "clusters_per_map_conn4": float(K4.mean()), "largest_count_conn8": int(K8.max())},
               "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d clouds" % B, "host_composition": host_result}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    if host_result:
        results["ratio_host_over_conn8_plane"] = host_result["ms_scaled_to_all_clouds"] / results["conn8_plane"]["ms_median"]
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
