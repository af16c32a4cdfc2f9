#!/usr/bin/env python3
"""gg_route_planes on the headline shape of tools/bench_fusion.py (1024 maps of 364 x 364).  The planes are those a drive leaves behind:
visibility_clouds on 1024 GG_POINT16 clouds of a 64-ring scan, fused by fuse_states over three frames with a non-zero index shift between
them; the goals are the frontier plane, the blocked plane is the fused state (occupied or never observed), and the cost plane is an
inflation of the clearance of the fused state (252 beside an obstacle, falling by 50 per cell of distance to 1).  fuse_states runs with
miss = 3 and free_threshold = -2, so that one free observation frees a cell: with the defaults of the fusion benchmark no cell of this
workload becomes free and there is nothing to route.  Timed by stream events, median of --reps with the warm-up excluded; ms per call:

  dist            (a) route_planes, the D plane alone
  all             (b) D + next + counts + the paths from the robot cell (max_path 1024)
  dist_bounded    (c) as (a) with max_cost = the median finite D of the unbounded field
  all_bounded     (d) as (b) with that max_cost
  copy            (e) one device-to-device copy that moves as many bytes as (b)'s algorithmic traffic (it reads half of them and writes
                  half): the bandwidth yardstick of this session
  one_map         (f) as (b) for n = 1: a single map runs on one compute unit -- a latency, measured and written down, not a target
  serpentine      (g) as (b) on 1024 one-cell-wide serpentines of the same size, the adversarial case for a tiled relaxation
  one_serpentine  (h) as (g) for n = 1
  robot_goal      (i) the reverse question: the robot cell of every map is its one goal (goal_planes), D + next + counts: the cost from
                  every free cell to the robot, read at the frontier cells by the caller

  host_dijkstra   the caller's alternative: download the three planes, build the graph (numpy, whole planes at a time), run
                  scipy.sparse.csgraph.dijkstra(..., min_only=True) per map, upload D -- on --sample maps, scaled to all of them.  Its D is
                  asserted equal to (a)'s on bits on that sample

Every repetition runs (a) (b) (c) (d) (e) (i); (f) (g) (h) run --reps-slow times behind them.  Needs a GPU; writes one JSON file and prints
it.  For times per kernel run the tool alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_route.py --reps 3`.

    python tools/bench_route.py --out profiles/route/summary.json
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

FUSE = dict(hit=4, miss=3, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)
ROUTE = dict(connectivity=8, straight=5, diagonal=7, cost_max=252)
DIRECTIONS = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))


def host_dijkstra(goals, blocked, cost):
    """D of one map on the host: the graph of the admissible steps built with whole-plane numpy operations, then scipy's Dijkstra from all
    goals at once.  Edge p -> q of weight s * w(p) for every admissible step q -> p"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    rows, cols = goals.shape
    open_ = np.zeros((rows + 2, cols + 2), bool)
    open_[1:-1, 1:-1] = blocked < 0
    w = np.clip(cost.astype(np.int64), 1, ROUTE["cost_max"])
    index = np.arange(rows * cols).reshape(rows, cols)
    src, dst, wt = [], [], []
    here = open_[1:-1, 1:-1]
    for k, (a, b) in enumerate(DIRECTIONS):
        ok = here & open_[1 + a:rows + 1 + a, 1 + b:cols + 1 + b]  # q and p = q + (a, b)
        if k >= 4:
            ok &= open_[1 + a:rows + 1 + a, 1:-1] & open_[1:-1, 1 + b:cols + 1 + b]
        q = index[ok]
        p = q + a * cols + b
        src.append(p)
        dst.append(q)
        wt.append((ROUTE["straight"] if k < 4 else ROUTE["diagonal"]) * w.ravel()[p])
    G = csr_matrix((np.concatenate(wt).astype(np.float64), (np.concatenate(src), np.concatenate(dst))), shape=(rows * cols, rows * cols))
    sources = np.flatnonzero(((goals >= 0) & here).ravel())
    if len(sources) == 0:
        return np.full((rows, cols), _lib.GG_ROUTE_NONE, np.int32)
    d = dijkstra(G, directed=True, indices=sources, min_only=True)  # (integer sums far below 2^53: exact in float64)
    return np.where(np.isinf(d), _lib.GG_ROUTE_NONE, d).astype(np.int32).reshape(rows, cols)


def serpentine(rows, cols):
    blocked = np.full((rows, cols), -1, np.int32)
    for r in range(1, rows, 2):
        blocked[r, :] = 0
        blocked[r, cols - 1 if (r // 2) % 2 == 0 else 0] = -1
    goals = np.full((rows, cols), -1, np.int32)
    goals[0, 0] = 0
    last = (rows - 1) // 2 * 2
    return goals, blocked, last * cols + (cols - 1 if (last // 2) % 2 == 0 else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-slow", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--max-path", type=int, default=1024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_route.py needs a GPU")
    B = args.maps
    base = [synth.hdl64_cloud(seed=3000 + k, n_az=args.n_az) for k in range(16)]
    stride = (max(len(c) for c in base) + 63) // 64 * 64
    host = np.zeros((16, stride), dtype=api.POINT16_DTYPE)
    for k, c in enumerate(base):
        host[k, : len(c)] = api.pack16(c)
    pts = torch.from_numpy(host.view(np.uint8).reshape(16, stride, 16)).cuda().repeat((B + 15) // 16, 1, 1)[:B].contiguous()
    n_pts = [len(base[b % 16]) for b in range(B)]
    origins, base_z = np.zeros((B, 3), np.float32), np.full(B, -1.73)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    rows, cols = seg.rows, seg.cols
    cells = rows * cols
    shifts = np.tile(np.array((3, -2), np.int32), (B, 1))
    robot = np.full(B, (rows // 2) * cols + cols // 2, np.int32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        # three frames of the same observations, scrolled against each other
        first = seg.fuse_states(states, on_torch_stream=True, **FUSE)
        second = seg.fuse_states(states, first.evidence, shifts=-shifts, on_torch_stream=True, **FUSE)
        fused = seg.fuse_states(states, second.evidence, shifts=shifts, on_torch_stream=True, **FUSE)
        goals, blocked = fused.frontier, fused.state
        clear = seg.clearance_planes(blocked, nearest=False, distance=False, on_torch_stream=True)
        cost = (252.0 - 50.0 * (clear.dist2.float().sqrt() - 1.0)).clamp_(1.0, 252.0).to(torch.int32).contiguous()
        del clear, first, second
        s_goals, s_blocked, s_start = serpentine(rows, cols)
        serp_goals = torch.from_numpy(s_goals).cuda()[None].repeat(B, 1, 1).contiguous()
        serp_blocked = torch.from_numpy(s_blocked).cuda()[None].repeat(B, 1, 1).contiguous()
        serp_starts = np.full(B, s_start, np.int32)

        full = seg.route_planes(goals, blocked, cost, starts=robot, max_path=args.max_path, on_torch_stream=True, **ROUTE)
        only = seg.route_planes(goals, blocked, cost, next=False, counts=False, on_torch_stream=True, **ROUTE)
        stream.synchronize()
        assert torch.equal(only.dist, full.dist)
        finite = full.dist[full.dist != _lib.GG_ROUTE_NONE]
        R = int(finite.median().item()) if finite.numel() else 1
        full_b = seg.route_planes(goals, blocked, cost, max_cost=R, starts=robot, max_path=args.max_path, on_torch_stream=True, **ROUTE)
        only_b = seg.route_planes(goals, blocked, cost, max_cost=R, next=False, counts=False, on_torch_stream=True, **ROUTE)
        one = seg.route_planes(goals[:1], blocked[:1], cost[:1], starts=robot[:1], max_path=args.max_path, on_torch_stream=True, **ROUTE)
        serp = seg.route_planes(serp_goals, serp_blocked, starts=serp_starts, max_path=args.max_path, on_torch_stream=True, **ROUTE)
        serp_one = seg.route_planes(serp_goals[:1], serp_blocked[:1], starts=serp_starts[:1], max_path=args.max_path, on_torch_stream=True, **ROUTE)
        robot_goals = api.goal_planes([[(rows // 2, cols // 2)]] * B, rows, cols, device="cuda")
        back = seg.route_planes(robot_goals, blocked, cost, on_torch_stream=True, **ROUTE)
        stream.synchronize()
        none = torch.full_like(full.dist, _lib.GG_ROUTE_NONE)
        assert torch.equal(full_b.dist, torch.where(full.dist <= R, full.dist, none)) and torch.equal(only_b.dist, full_b.dist)
        assert torch.equal(one.dist[0], full.dist[0]) and torch.equal(serp_one.dist[0], serp.dist[0])
        corridors = (rows + 1) // 2
        assert int(serp.path_len[0].item()) == corridors * cols + corridors - 1 and int(serp.counts[0, 1].item()) == int(serp.counts[0, 2].item())
        del none

        # the caller's alternative, on a sample of maps
        sample = sorted({int(i) for i in np.linspace(0, B - 1, min(args.sample, B))})
        t_host = []
        host_dijkstra(goals[0].cpu().numpy(), blocked[0].cpu().numpy(), cost[0].cpu().numpy())  # (warm-up: scipy's import and first call)
        for i in sample:
            stream.synchronize()
            t0 = time.perf_counter()
            g, b, c = goals[i].cpu().numpy(), blocked[i].cpu().numpy(), cost[i].cpu().numpy()
            d = host_dijkstra(g, b, c)
            up = torch.from_numpy(d).cuda()
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(up, full.dist[i]), f"map {i}: the host Dijkstra and route_planes differ"
        cnt = full.counts.double().mean(0).tolist()
        plen = full.path_len.double()
        traffic = B * cells * 4 * 5  # per cell: goals, blocked and cost read, D and next written
        src = torch.empty(traffic // 8, dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        shape = {"maps": B, "rows": rows, "cols": cols, "fuse_params": FUSE, "route_params": ROUTE, "max_cost_bounded": R, "max_path": args.max_path,
                 "goals_per_map": cnt[0], "reached_cells_per_map": cnt[1], "unblocked_cells_per_map": cnt[2],
                 "reached_cells_per_map_bounded": float(full_b.counts[:, 1].double().mean().item()),
                 "path_cells_mean": float(plen.mean().item()), "path_cells_max": float(plen.max().item()), "maps_with_a_path": int((plen > 0).sum().item()),
                 "serpentine_path_cells": int(serp.path_len[0].item()), "robot_goal_reached_cells_per_map": float(back.counts[:, 1].double().mean().item()),
                 "algorithmic_bytes_all": traffic, "algorithmic_bytes_dist": traffic * 4 // 5, "copy_bytes_read_plus_written": int(src.numel()) * 8}

        def run(what):
            if what == "dist":
                seg.route_planes(goals, blocked, cost, next=False, counts=False, out=only, on_torch_stream=True, **ROUTE)
            elif what == "all":
                seg.route_planes(goals, blocked, cost, starts=robot, max_path=args.max_path, out=full, on_torch_stream=True, **ROUTE)
            elif what == "dist_bounded":
                seg.route_planes(goals, blocked, cost, max_cost=R, next=False, counts=False, out=only_b, on_torch_stream=True, **ROUTE)
            elif what == "all_bounded":
                seg.route_planes(goals, blocked, cost, max_cost=R, starts=robot, max_path=args.max_path, out=full_b, on_torch_stream=True, **ROUTE)
            elif what == "robot_goal":
                seg.route_planes(robot_goals, blocked, cost, out=back, on_torch_stream=True, **ROUTE)
            elif what == "copy":
                dst.copy_(src)
            elif what == "one_map":
                seg.route_planes(goals[:1], blocked[:1], cost[:1], starts=robot[:1], max_path=args.max_path, out=one, on_torch_stream=True, **ROUTE)
            elif what == "serpentine":
                seg.route_planes(serp_goals, serp_blocked, starts=serp_starts, max_path=args.max_path, out=serp, on_torch_stream=True, **ROUTE)
            else:
                seg.route_planes(serp_goals[:1], serp_blocked[:1], starts=serp_starts[:1], max_path=args.max_path, out=serp_one, on_torch_stream=True, **ROUTE)

        events = {}

        def timed(what, keep):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(what)
            e1.record()
            if keep:
                events.setdefault(what, []).append((e0, e1))

        for rep in range(-args.warmup, args.reps):
            for what in ("dist", "all", "dist_bounded", "all_bounded", "copy", "robot_goal"):
                timed(what, rep >= 0)
        stream.synchronize()
        for rep in range(-1, args.reps_slow):
            for what in ("one_map", "serpentine", "one_serpentine"):
                timed(what, rep >= 0)
        stream.synchronize()  # (once per group: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "reps_slow": args.reps_slow, "warmup": args.warmup, "unit": "ms per call", "host_dijkstra_equals_dist_on_the_sample": True}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    results["host_dijkstra"] = {"sample": sample, "ms_per_map": t_host, "ms_per_map_median": float(np.median(t_host)), "ms_scaled_to_all_maps": float(np.median(t_host)) * B}
    results["ratio_host_dijkstra_over_dist"] = results["host_dijkstra"]["ms_scaled_to_all_maps"] / results["dist"]["ms_median"]
    results["ratio_all_over_copy"] = results["all"]["ms_median"] / results["copy"]["ms_median"]
    results["ratio_dist_over_copy"] = results["dist"]["ms_median"] / results["copy"]["ms_median"]
    results["ratio_all_over_dist"] = results["all"]["ms_median"] / results["dist"]["ms_median"]
    results["ratio_dist_bounded_over_dist"] = results["dist_bounded"]["ms_median"] / results["dist"]["ms_median"]
    results["ratio_serpentine_over_all"] = results["serpentine"]["ms_median"] / results["all"]["ms_median"]
    results["copy_GBps"] = shape["copy_bytes_read_plus_written"] / results["copy"]["ms_median"] / 1e6
    results["all_us_per_map"] = results["all"]["ms_median"] * 1e3 / B
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
