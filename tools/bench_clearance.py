#!/usr/bin/env python3
"""gg_clearance_clouds on the headline shape of tools/bench_cluster.py (1024 GG_POINT16 clouds of a 64-ring scan on 364 x 364 maps, labels
from one default batch), timed by stream events, median of --reps with the warm-up excluded, the arms alternating inside every repetition;
ms per 1024 clouds:

  clouds_dist2       clearance_clouds, dist2 and the counts alone (nearest=False, distance=False), open band, min_points 1
  clouds_all         clearance_clouds with all outputs
  clouds_all_r30     clouds_all with max_cells = 30
  planes_all         clearance_planes on the id planes of cluster_clouds (connectivity 8, no table, no per-point ids), all outputs
  cluster_plane      that cluster_clouds call alone, for scale

and what a caller does today for the same field, timed by the wall clock on a SAMPLE of --host-maps maps and scaled up to the 1024 (the
output says so): cluster_clouds, the id planes to the host, scipy.ndimage.distance_transform_edt(return_indices=True) per map, the squared
distances and the indices back to the device.  Its dist2 is asserted bit-equal to clouds_all's on the sampled maps before anything is timed.
Needs a GPU; writes one JSON file and prints it.  For times per kernel run the tool alone under
`rocprofv3 --kernel-trace --stats -- python tools/bench_clearance.py --reps 3`.

    python tools/bench_clearance.py --out profiles/clearance/summary.json
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

from groundgrid_amd import _lib, api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--host-maps", type=int, default=32)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_clearance.py needs a GPU")
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
    arms = {"clouds_dist2": dict(nearest=False, distance=False), "clouds_all": dict(), "clouds_all_r30": dict(max_cells=30)}
    cluster_kw = dict(connectivity=8, max_clusters=0, point_clusters=False)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        outs = {name: seg.clearance_clouds(pts, n_pts, labels=batch.labels, **kw) for name, kw in arms.items()}  # (the first call allocates)
        clusters = seg.cluster_clouds(pts, n_pts, labels=batch.labels, **cluster_kw)
        outs["planes_all"] = seg.clearance_planes(clusters.cell_cluster)
        stream.synchronize()
        same_modes = all(bool(torch.equal(getattr(outs["planes_all"], k), getattr(outs["clouds_all"], k))) for k in ("dist2", "nearest", "distance", "n_occupied"))
        assert same_modes, "clearance_planes on the cluster planes differs from clearance_clouds"
        occupied = outs["clouds_all"].n_occupied.cpu().numpy()
        d2 = outs["clouds_all"].dist2
        found = d2 != _lib.GG_CLEARANCE_NONE
        shape = {"clouds": B, "rows": rows, "cols": cols, "points_per_cloud": int(np.mean(n_pts)), "point_format": "GG_POINT16",
                 "input_points": int(np.sum(n_pts)), "occupied_cells_per_map": float(occupied.mean()),
                 "dist2_mean": float(d2[found].double().mean().item()), "dist2_max": int(d2[found].max().item())}

        # what a caller does today, on the first host-maps maps
        H = min(args.host_maps, B)
        host_result = None
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None and H > 0:

            def host_arm():
                planes = seg.cluster_clouds(pts[:H], n_pts[:H], labels=batch.labels[:H], **cluster_kw).cell_cluster.cpu().numpy()
                dist2, index = np.empty((H, rows, cols), np.int32), np.empty((H, rows, cols), np.int32)
                for b in range(H):
                    free = planes[b] < 0
                    if free.all():  # (scipy gives the distance to the border of the array then; the field says "none")
                        dist2[b], index[b] = _lib.GG_CLEARANCE_NONE, -1
                        continue
                    edt, idx = ndimage.distance_transform_edt(free, return_indices=True)
                    dist2[b] = np.rint(edt * edt)
                    index[b] = idx[0] * cols + idx[1]
                return torch.from_numpy(dist2).cuda(), torch.from_numpy(index).cuda()

            host_d2, _ = host_arm()
            assert bool(torch.equal(host_d2, outs["clouds_all"].dist2[:H])), "dist2 differs from scipy.ndimage.distance_transform_edt on the sampled maps"
            walls = []
            for _ in range(args.host_reps):
                stream.synchronize()
                t0 = time.perf_counter()
                host_arm()
                stream.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
            host_result = {"note": "wall clock on a sample of %d maps, scaled up to %d by %g" % (H, B, B / H), "maps": H,
                           "ms_median_measured": float(np.median(walls)), "ms_scaled_to_all_clouds": float(np.median(walls)) * B / H,
                           "dist2_equals_clouds_all": True}

        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in list(arms) + ["planes_all", "cluster_plane"]:  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "cluster_plane":
                    seg.cluster_clouds(pts, n_pts, labels=batch.labels, out=clusters, **cluster_kw)
                elif what == "planes_all":
                    seg.clearance_planes(clusters.cell_cluster, out=outs[what])
                else:
                    seg.clearance_clouds(pts, n_pts, labels=batch.labels, out=outs[what], **arms[what])
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d clouds" % B, "seed_mode_equals_cloud_mode": same_modes,
               "host_composition": host_result}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    if host_result:
        results["ratio_host_over_clouds_all"] = host_result["ms_scaled_to_all_clouds"] / results["clouds_all"]["ms_median"]
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
