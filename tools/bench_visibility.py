#!/usr/bin/env python3
"""gg_visibility_clouds on the headline shape of tools/bench_cluster.py (1024 GG_POINT16 clouds of a 64-ring scan on 364 x 364 maps, labels
from one default batch, the sensor in the middle of every map), timed by stream events, median of --reps with the warm-up excluded, the arms
alternating inside every repetition; ms per 1024 clouds:

  state              visibility_clouds, the state planes alone (counts=False), open band, min_points 1
  state_counts       ... with the counts
  state_counts_r30   state_counts with max_cells = 30
  chain              state_counts, then clearance_planes on the state planes (all outputs): the conservative clearance of a costmap
  cluster_plane      cluster_clouds with planes and counts only (connectivity 8, no table, no per-point ids): the LOWER BOUND, because
                     visibility_clouds contains its occupancy launches

and what a caller does today for the same planes, timed by the wall clock on a SAMPLE of --host-maps maps and scaled up to the 1024 (the
output says so): the numpy restatement of the definition (tests/visibility_ref.expected_visibility) per map, on an occupancy and a set of
hit cells that are already on the host.  Its planes and counts are asserted bit-equal to state_counts' on the sampled maps before anything
is timed.  Needs a GPU; writes one JSON file and prints it.  For times per kernel run the tool alone under
`rocprofv3 --kernel-trace --stats -- python tools/bench_visibility.py --reps 3`.

    python tools/bench_visibility.py --out profiles/visibility/summary.json
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
    ap.add_argument("--host-maps", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_visibility.py needs a GPU")
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
    arms = {"state": dict(counts=False), "state_counts": dict(), "state_counts_r30": dict(max_cells=30)}
    cluster_kw = dict(connectivity=8, max_clusters=0, point_clusters=False)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        outs = {name: seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, **kw) for name, kw in arms.items()}  # (the first call allocates)
        outs["chain"] = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels)
        field = seg.clearance_planes(outs["chain"].state)
        clusters = seg.cluster_clouds(pts, n_pts, labels=batch.labels, **cluster_kw)
        stream.synchronize()
        assert bool(torch.equal(outs["state"].state, outs["state_counts"].state)) and bool(torch.equal(outs["chain"].state, outs["state_counts"].state))
        assert bool(torch.equal(outs["state_counts"].state == 1, clusters.cell_cluster >= 0)), "the occupied cells are not those of cluster_clouds"
        counts = outs["state_counts"].counts.cpu().numpy()
        assert np.all(counts.sum(axis=1) == rows * cols)
        shape = {"clouds": B, "rows": rows, "cols": cols, "points_per_cloud": int(np.mean(n_pts)), "point_format": "GG_POINT16",
                 "input_points": int(np.sum(n_pts)), "free_cells_per_map": float(counts[:, 0].mean()), "unknown_cells_per_map": float(counts[:, 1].mean()),
                 "occupied_cells_per_map": float(counts[:, 2].mean()), "free_cells_per_map_r30": float(outs["state_counts_r30"].counts[:, 0].double().mean().item())}

        # what a caller does today, on the first host-maps maps: the numpy restatement of the definition per map
        H = min(args.host_maps, B)
        host_result = None
        if H > 0:
            from oracle import oracle
            from tests import visibility_ref

            hits = seg.rasterize_clouds(pts[:H], n_pts[:H], labels=batch.labels[:H], channels=["nonground_count", "ground_count"]).sum(dim=1).cpu().numpy() > 0
            occupied = clusters.cell_cluster[:H].cpu().numpy() >= 0
            inside, r0, c0 = oracle.OracleMap(120.0, 0.33).get_index(0.0, 0.0)
            assert inside
            rays = [int(h.sum()) for h in hits]
            steps = [int(np.maximum(np.abs(np.argwhere(h)[:, 0] - r0), np.abs(np.argwhere(h)[:, 1] - c0)).sum()) for h in hits]

            def host_arm():
                return [visibility_ref.expected_visibility(occupied[b], hits[b], (r0, c0), 0, "row") for b in range(H)]

            got_state, got_counts = outs["state_counts"].state[:H].cpu().numpy(), counts[:H]
            for b, (state, cnt) in enumerate(host_arm()):
                assert np.array_equal(state, got_state[b]) and np.array_equal(cnt, got_counts[b]), f"map {b} differs from the numpy reference"
            walls = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                host_arm()
                walls.append((time.perf_counter() - t0) * 1e3)
            host_result = {"note": "numpy reference (tests/visibility_ref.py) on this host's CPU, wall clock on a sample of %d maps, scaled up to %d by %g; "
                                   "occupancy and hit cells already on the host" % (H, B, B / H), "maps": H,
                           "ms_median_measured": float(np.median(walls)), "ms_per_map": float(np.median(walls)) / H,
                           "ms_scaled_to_all_clouds": float(np.median(walls)) * B / H, "equals_state_counts": True,
                           "rays_per_map": float(np.mean(rays)), "ray_steps_per_map": float(np.mean(steps))}

        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in list(arms) + ["chain", "cluster_plane"]:  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "cluster_plane":
                    seg.cluster_clouds(pts, n_pts, labels=batch.labels, out=clusters, **cluster_kw)
                elif what == "chain":
                    seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, out=outs[what])
                    seg.clearance_planes(outs[what].state, out=field)
                else:
                    seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, out=outs[what], **arms[what])
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d clouds" % B, "host_reference": host_result}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    results["ratio_state_counts_over_cluster_plane"] = results["state_counts"]["ms_median"] / results["cluster_plane"]["ms_median"]
    if host_result:
        results["ratio_host_over_state_counts"] = host_result["ms_scaled_to_all_clouds"] / results["state_counts"]["ms_median"]
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
