#!/usr/bin/env python3
"""gg_route_headings on the headline shape of tools/bench_footprint.py (1024 maps of 364 x 364).  The heading masks are footprint_planes of
that benchmark's car of 4.7 m x 1.9 m at the K headings of the move table, on the fused states of the drive of tools/bench_route.py
(visibility_clouds on 1024 GG_POINT16 clouds of a 64-ring scan, fused by fuse_states over three frames with a non-zero index shift between
them and miss = 3: with the fusion parameters of tools/bench_footprint.py the car fits nowhere near a frontier and nothing is routed).  The
goal cells are those within 16 cells of the frontier plane of that fusion (clearance_planes with the frontier as seeds): on a frontier
cell itself the car never fits, its footprint covers the unknown cells beside it.  The moves are heading_moves(step 2, unit 10, turn 3, reverse 150 %) at K = 16; no cost
plane (w = 1): at this size the overflow limit leaves cost_max <= 26 at K = 16 and <= 13 at K = 32, which the shape block records.
Timed by stream events, median of --reps with the warm-up excluded; ms per call:

  dist            (a) route_headings, the K planes of D alone
  all             (b) D + next + best + best_heading + counts + the paths from the robot pose (the middle cell, heading 0; max_len 1024)
  dist_bounded    (c) as (a) with max_cost = the median finite D of the unbounded field
  dist_k8, dist_k32  (d) as (a) with 8 and with 32 headings (masks of their own from footprint_planes)
  dist_forward    (e) as (a) without the reverse moves
  one_map         (f) as (b) for n = 1: a single map runs on one compute unit -- a latency, measured and written down, not a target
  copy            (g) one device-to-device copy that moves as many bytes as (b)'s algorithmic traffic (it reads half of them and writes
                  half): the bandwidth yardstick of this session
  route_planes    (h) gg_route_planes (connectivity 8, straight 10, diagonal 14, D alone) on the min_fit = 1 projection of the same masks: the
                  2-D floor, which this call costs roughly K times

  host_dijkstra   (i) the caller's alternative: download the mask and the goals, build the graph of (cell, heading) states (numpy, whole
                  planes at a time), run scipy.sparse.csgraph.dijkstra(..., min_only=True) per map, upload D -- on --sample maps, SCALED to
                  all of them.  Its D is asserted equal to (a)'s on bits on that sample

The slow arms would make ten repetitions long, so the tool times one warm-up round and then runs as many repetitions (at most --reps) as
fit --budget-s; the number it ran is in the output.  Needs a GPU; writes one JSON file and prints it.  For times per kernel run the tool
alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_headings.py --reps 2 --sample 0`.

    python tools/bench_headings.py --out profiles/headings/summary.json
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

FUSE = dict(hit=4, miss=3, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)  # tools/bench_route.py: one free observation frees a cell
CAR = dict(ahead=11.2, behind=3.0, left=2.9, right=2.9)
MOVES = dict(step=2, unit=10, turn=3, reverse_pct=150)


def host_dijkstra(mask, goals, moves):
    """D of one map on the host, int32 [K, rows, cols] (w = 1, any goal heading): the graph of the admissible moves built with whole-plane
    numpy operations, then scipy's Dijkstra from all goal states at once.  Edge (k2, p) -> (k, q) of weight s for every admissible move
    (k, q) -> (k2, p); of two moves between the same states the cheaper stays"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra

    K = moves.shape[0]
    rows, cols = goals.shape
    n = K * rows * cols
    adm = np.stack([((mask.view(np.uint32) >> k) & 1).astype(bool) for k in range(K)])
    index = np.arange(rows * cols).reshape(rows, cols)
    src, dst, wt = [], [], []
    for k in range(K):
        for da, db, k2, s in moves[k].tolist():
            if not s:
                continue
            r0, r1, c0, c1 = max(0, -da), min(rows, rows - da), max(0, -db), min(cols, cols - db)
            ok = adm[k, r0:r1, c0:c1] & adm[k2, r0 + da:r1 + da, c0 + db:c1 + db]
            q = index[r0:r1, c0:c1][ok]
            src.append(k2 * rows * cols + q + da * cols + db)
            dst.append(k * rows * cols + q)
            wt.append(np.full(len(q), s, np.int64))
    src, dst, wt = np.concatenate(src), np.concatenate(dst), np.concatenate(wt)
    order = np.lexsort((wt, dst, src))
    src, dst, wt = src[order], dst[order], wt[order]
    first = np.ones(len(src), bool)
    first[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    G = coo_matrix((wt[first].astype(np.float64), (src[first], dst[first])), shape=(n, n)).tocsr()
    sources = np.flatnonzero((adm & (goals >= 0)[None]).ravel())
    if len(sources) == 0:
        return np.full((K, rows, cols), _lib.GG_ROUTE_NONE, np.int32)
    d = dijkstra(G, directed=True, indices=sources, min_only=True)  # (integer sums far below 2^53: exact in float64)
    return np.where(np.isinf(d), _lib.GG_ROUTE_NONE, d).astype(np.int32).reshape(K, rows, cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget-s", type=float, default=240.0)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--goal-reach", type=int, default=16, help="a goal cell lies within this many cells of a frontier cell")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_headings.py needs a GPU")
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
    tables = {K: api.rotation_table(2.0 * np.pi * np.arange(K) / K) for K in (8, 16, 32)}
    moves = {K: api.heading_moves(tables[K], **MOVES) for K in tables}
    forward = api.heading_moves(tables[16], **dict(MOVES, reverse_pct=0))
    limits = {K: int(_lib.GG_HEADINGS_LIMIT // (int(moves[K][:, :, 3].max()) * cells * K)) for K in tables}
    robot = np.tile(np.array(((rows // 2) * cols + cols // 2, 0), np.int32), (B, 1))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        # three frames of the same observations, scrolled against each other (tools/bench_route.py)
        first = seg.fuse_states(states, on_torch_stream=True, **FUSE)
        second = seg.fuse_states(states, first.evidence, shifts=-shifts, on_torch_stream=True, **FUSE)
        fused = seg.fuse_states(states, second.evidence, shifts=shifts, on_torch_stream=True, **FUSE)
        blocked = fused.state
        # the car never fits ON a frontier cell (its footprint would cover the unknown cells beside it), so the goal cells are those within
        # --goal-reach cells of the frontier: as near to it as a vehicle of that length gets
        near = seg.clearance_planes(fused.frontier, nearest=False, distance=False, on_torch_stream=True)
        goals = torch.where(near.dist2 <= args.goal_reach ** 2, 0, -1).to(torch.int32).contiguous()
        del first, second, near
        masks, fit = {}, None
        for K in tables:
            fp = seg.footprint_planes(blocked, api.footprint_spans(tables[K], **CAR, radius=14), min_fit=1, counts=False, on_torch_stream=True)
            masks[K] = fp.mask
            fit = fp.fit if K == 16 else fit
        args_of = {"dist": (16, moves[16], {}), "dist_k8": (8, moves[8], {}), "dist_k32": (32, moves[32], {}), "dist_forward": (16, forward, {})}
        outs = {}
        t0 = time.perf_counter()
        for what, (K, table, kw) in args_of.items():
            outs[what] = seg.route_headings(masks[K], goals, table, cost_max=1, next=False, best=False, counts=False, on_torch_stream=True, **kw)
        outs["all"] = seg.route_headings(masks[16], goals, moves[16], cost_max=1, starts=robot, max_len=args.max_len, on_torch_stream=True)
        stream.synchronize()
        first_round_s = time.perf_counter() - t0
        assert torch.equal(outs["all"].dist, outs["dist"].dist)
        part = outs["dist"].dist[: min(B, 64)]  # (the median of the first 64 maps' finite words: every map holds the same 16 scans in turn)
        finite = part[part != _lib.GG_ROUTE_NONE]
        R = int(finite.float().median().item()) if finite.numel() else 1
        del part
        del finite
        outs["dist_bounded"] = seg.route_headings(masks[16], goals, moves[16], cost_max=1, max_cost=R, next=False, best=False, counts=False, on_torch_stream=True)
        outs["one_map"] = seg.route_headings(masks[16][:1], goals[:1], moves[16], cost_max=1, starts=robot[:1], max_len=args.max_len, on_torch_stream=True)
        flat = seg.route_planes(goals, fit, connectivity=8, straight=10, diagonal=14, cost_max=1, next=False, counts=False, on_torch_stream=True)
        stream.synchronize()
        assert torch.equal(outs["one_map"].dist[0], outs["all"].dist[0])
        none = _lib.GG_ROUTE_NONE
        assert torch.equal(outs["dist_bounded"].dist, torch.where(outs["dist"].dist <= R, outs["dist"].dist, torch.full_like(outs["dist"].dist, none)))

        # the caller's alternative, on a sample of maps
        sample = sorted({int(i) for i in np.linspace(0, B - 1, min(args.sample, B))}) if args.sample > 0 else []
        t_host = []
        for j, i in enumerate(sample[:1] + sample):  # (the first pass is the warm-up: scipy's import and first call)
            stream.synchronize()
            t0 = time.perf_counter()
            m, g = masks[16][i].cpu().numpy(), goals[i].cpu().numpy()
            d = host_dijkstra(m, g, moves[16])
            up = torch.from_numpy(d).cuda()
            torch.cuda.synchronize()
            if j > 0:
                t_host.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(up, outs["dist"].dist[i]), f"map {i}: the host Dijkstra and route_headings differ"
        cnt = outs["all"].counts.double().mean(0).tolist()
        assert cnt[0] > 0 and cnt[1] > cnt[0], "the scene has no goal state or nothing to route"
        plen = outs["all"].path_len.double()
        traffic = B * cells * (16 + 8 * 16)  # per cell: mask and goals read, best and best_heading written, 16 words of D and of next written
        src = torch.empty(traffic // 8, dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        shape = {"maps": B, "rows": rows, "cols": cols, "fuse_params": FUSE, "car": CAR, "moves": MOVES, "cost_plane": None, "cost_max": 1, "goal_reach_cells": args.goal_reach,
                 "largest_cost_max_the_limit_allows": limits, "max_cost_bounded": R, "max_len": args.max_len,
                 "goal_states_per_map": cnt[0], "reached_states_per_map": cnt[1], "admissible_states_per_map": cnt[2],
                 "reached_states_per_map_bounded": float((outs["dist_bounded"].dist != none).sum().item()) / B,
                 "reached_cells_per_map_route_planes": float((flat.dist != none).sum().item()) / B,
                 "reached_cells_per_map_best": float((outs["all"].best != none).sum().item()) / B,
                 "path_states_mean": float(plen.mean().item()), "path_states_max": float(plen.max().item()), "maps_with_a_path": int((plen > 0).sum().item()),
                 "algorithmic_bytes_all": traffic, "copy_bytes_read_plus_written": int(src.numel()) * 8}

        def run(what):
            if what in args_of:
                K, table, kw = args_of[what]
                seg.route_headings(masks[K], goals, table, cost_max=1, next=False, best=False, counts=False, out=outs[what], on_torch_stream=True, **kw)
            elif what == "all":
                seg.route_headings(masks[16], goals, moves[16], cost_max=1, starts=robot, max_len=args.max_len, out=outs[what], on_torch_stream=True)
            elif what == "dist_bounded":
                seg.route_headings(masks[16], goals, moves[16], cost_max=1, max_cost=R, next=False, best=False, counts=False, out=outs[what], on_torch_stream=True)
            elif what == "one_map":
                seg.route_headings(masks[16][:1], goals[:1], moves[16], cost_max=1, starts=robot[:1], max_len=args.max_len, out=outs[what], on_torch_stream=True)
            elif what == "route_planes":
                seg.route_planes(goals, fit, connectivity=8, straight=10, diagonal=14, cost_max=1, next=False, counts=False, out=flat, on_torch_stream=True)
            else:
                dst.copy_(src)

        events = {}
        arms = ("dist", "all", "dist_bounded", "dist_k8", "dist_k32", "dist_forward", "one_map", "copy", "route_planes")
        # one round costs about what the first five calls took, twice (nine arms, of which all but three are as long as those)
        reps = int(max(1, min(args.reps, args.budget_s / max(2.0 * first_round_s, 1e-3) - args.warmup)))
        for rep in range(-args.warmup, reps):
            for what in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(what)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": reps, "reps_asked": args.reps, "warmup": args.warmup, "unit": "ms per call", "host_dijkstra_equals_dist_on_the_sample": bool(sample)}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    if t_host:
        results["host_dijkstra"] = {"sample": sample, "ms_per_map": t_host, "ms_per_map_median": float(np.median(t_host)),
                                    "ms_scaled_to_all_maps": float(np.median(t_host)) * B, "scaled": True}
        results["ratio_host_dijkstra_scaled_over_dist"] = results["host_dijkstra"]["ms_scaled_to_all_maps"] / results["dist"]["ms_median"]
    results["ratio_all_over_copy"] = results["all"]["ms_median"] / results["copy"]["ms_median"]
    results["ratio_all_over_dist"] = results["all"]["ms_median"] / results["dist"]["ms_median"]
    results["ratio_dist_over_route_planes"] = results["dist"]["ms_median"] / results["route_planes"]["ms_median"]
    results["ratio_dist_k32_over_dist_k8"] = results["dist_k32"]["ms_median"] / results["dist_k8"]["ms_median"]
    results["copy_GBps"] = shape["copy_bytes_read_plus_written"] / results["copy"]["ms_median"] / 1e6
    results["dist_us_per_map"] = results["dist"]["ms_median"] * 1e3 / B
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
