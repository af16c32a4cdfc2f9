#!/usr/bin/env python3
"""gg_cluster_planes on 1024 maps of 364 x 364, timed by stream events, median of --reps with the warm-up excluded, the arms alternating
inside every repetition; ms per 1024 maps.  The planes are those of the chain as the other tools build it: the clouds of
tools/bench_cluster.py (1024 GG_POINT16 clouds of a 64-ring scan, labels from one default batch), the observation planes of
tools/bench_fusion.py fused over three frames as tools/bench_route.py fuses them (miss 3, so that free cells and a frontier exist), and D
of route_planes from the robot cell.

  dense_occ       (a) the fused state planes, lo = hi = 1 (the occupied cells), connectivity 8, heads and a table of 256
  dense_blocked   (a) ... lo = 0 (occupied or never observed): the blocked plane of the chain
  frontier_m1     (b) the frontier planes, values = D, min_cells 1 (no size plane: the size and filter launches do not run)
  frontier_m5     (b) ... min_cells 5 (with the size plane and the filter)
  sparse          (c) the id planes of gg_cluster_clouds with lo = 0, plane and heads alone
  cluster_plane       gg_cluster_clouds' "plane and counts alone" arm (conn8_plane of tools/bench_cluster.py) in the same run: (c) runs a
                      strict subset of its launches
  spirals             1024 one-cell-wide spirals (cluster_ref.spiral), the longest chains: reported, not bounded
  <arm>_tile          each of the six with the tile-local stage (debug_regions_tile(1)): 32 x 32 tiles labelled in LDS in
                      front of the flatten, the seams united through global atomics; its outputs are compared with the plain path's first
  copy_28 / _32 / _52 one device-to-device copy that moves as many bytes as the algorithmic traffic of a call with 28 (plane, heads,
                      table), 32 (with values) or 52 (with values, sizes and the filter) bytes per cell; it reads half and writes half

and what a caller does today for the same planes, by the wall clock on --host-maps maps and scaled to the 1024: the planes to the host,
scipy.ndimage.label + bincount + a sequential relabel per map, the id planes back to the device.  Its planes are compared with the call's
bit for bit before anything is timed.  --arms names the arms to run (default: all).  Needs a GPU; writes one JSON file and prints it.
For times per kernel run one arm alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_regions.py --reps 3 --host-maps 0
--arms dense_occ`.

    python tools/bench_regions.py --out profiles/regions/summary.json
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

FUSE = dict(hit=4, miss=3, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)  # tools/bench_route.py
ROUTE = dict(connectivity=8, straight=5, diagonal=7, cost_max=252)
REGION_ARMS = ("dense_occ", "dense_blocked", "frontier_m1", "frontier_m5", "sparse", "spirals")
TILE_ARMS = tuple(a + "_tile" for a in REGION_ARMS)  # the same calls with the tile-local stage (debug_regions_tile(1))
ALL_ARMS = tuple(x for pair in zip(REGION_ARMS, TILE_ARMS) for x in pair) + ("cluster_plane", "copy_28", "copy_32", "copy_52")


def spiral_plane(rows, cols):
    """tests/cluster_ref.spiral without the tests: a one-cell-wide path from the corner inwards, a free lane between its turns"""
    occ = np.zeros((rows, cols), dtype=bool)
    r, c, dr, dc = 0, 0, 0, 1
    occ[0, 0] = True

    def can_step(rr, cc, ddr, ddc):
        r1, c1, r2, c2 = rr + ddr, cc + ddc, rr + 2 * ddr, cc + 2 * ddc
        if not (0 <= r1 < rows and 0 <= c1 < cols) or occ[r1, c1]:
            return False
        return not (0 <= r2 < rows and 0 <= c2 < cols) or not occ[r2, c2]

    for _ in range(rows * cols):  # (bounded: every step marks a new cell)
        if not can_step(r, c, dr, dc):
            dr, dc = dc, -dr
            if not can_step(r, c, dr, dc):
                break
        r, c = r + dr, c + dc
        occ[r, c] = True
    return np.where(occ, 0, -1).astype(np.int32)


def host_regions(torch, ndimage, seeds, lo, hi, connectivity, min_cells):
    """what a caller composes today; returns the id planes on the device"""
    grid = seeds.cpu().numpy()
    structure = np.ones((3, 3), dtype=np.int32) if connectivity == 8 else None
    out = np.empty(grid.shape, dtype=np.int32)
    for b in range(grid.shape[0]):
        lab, n = ndimage.label((grid[b] >= lo) & (grid[b] <= hi), structure=structure)
        size = np.bincount(lab.ravel(), minlength=n + 1)
        keep = size >= min_cells
        keep[0] = False
        new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)  # (scipy numbers in raster order: the order of the smallest index)
        out[b] = new[lab]
    return torch.from_numpy(out).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--host-maps", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--max-regions", type=int, default=256)
    ap.add_argument("--arms", nargs="*", default=list(ALL_ARMS), choices=ALL_ARMS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_regions.py needs a GPU")
    B, M, INT32_MAX = args.maps, args.max_regions, 0x7FFFFFFF
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
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        first = seg.fuse_states(states, on_torch_stream=True, **FUSE)
        second = seg.fuse_states(states, first.evidence, shifts=-shifts, on_torch_stream=True, **FUSE)
        fused = seg.fuse_states(states, second.evidence, shifts=shifts, on_torch_stream=True, **FUSE)
        del first, second, states
        robot_goals = api.goal_planes([[(rows // 2, cols // 2)]] * B, rows, cols, device="cuda")
        D = seg.route_planes(robot_goals, fused.state, next=False, counts=False, on_torch_stream=True, **ROUTE).dist
        del robot_goals
        cluster_kw = dict(connectivity=8, max_clusters=0, point_clusters=False)
        ids = seg.cluster_clouds(pts, n_pts, labels=batch.labels, **cluster_kw)  # (on the context's stream: ordered by the library)
        spirals = torch.from_numpy(spiral_plane(rows, cols)).cuda()[None].repeat(B, 1, 1).contiguous()
        stream.synchronize()
        seg.synchronize()
        calls = {"dense_occ": (fused.state, dict(lo=1, hi=1, max_regions=M)),
                 "dense_blocked": (fused.state, dict(lo=0, max_regions=M)),
                 "frontier_m1": (fused.frontier, dict(values=D, max_regions=M)),
                 "frontier_m5": (fused.frontier, dict(values=D, min_cells=5, max_regions=M)),
                 "sparse": (ids.cell_cluster, dict(max_regions=0)),
                 "spirals": (spirals, dict(max_regions=M))}
        for name in REGION_ARMS:
            calls[name + "_tile"] = calls[name]
        outs = {}
        for name, (s, kw) in calls.items():
            if name in args.arms:
                seg.debug_regions_tile(1 if name.endswith("_tile") else 0)
                outs[name] = seg.cluster_planes(s, on_torch_stream=True, **kw)
        stream.synchronize()
        for name in REGION_ARMS:  # the two paths give the same bits
            if name in outs and name + "_tile" in outs:
                p, q = outs[name], outs[name + "_tile"]
                assert all(torch.equal(getattr(p, f), getattr(q, f)) for f in ("cell_cluster", "cell_size", "heads") if getattr(p, f) is not None), name
                if p.regions is not None:  # (the records at and beyond K are never written)
                    written = torch.arange(M, device="cuda")[None, :] < p.heads[:, :1]
                    assert torch.equal(p.regions[written], q.regions[written]), name
        shape = {"maps": B, "rows": rows, "cols": cols, "max_regions": M, "fuse": FUSE,
                 "occupied_fraction": float((fused.state == 1).float().mean().item()), "blocked_fraction": float((fused.state >= 0).float().mean().item()),
                 "frontier_cells_per_map": float((fused.frontier >= 0).sum().item()) / B,
                 "sparse_member_cells_per_map": float((ids.cell_cluster >= 0).sum().item()) / B}
        for name, res in outs.items():
            h = res.heads.double().mean(0).tolist()
            shape[name] = {"regions_per_map": h[0], "dropped_per_map": h[1], "member_cells_per_map": h[2], "kept_cells_per_map": h[3],
                           "largest_region_count": int(res.heads[:, 0].max().item())}
        if "sparse" in outs:
            assert torch.equal(outs["sparse"].cell_cluster, ids.cell_cluster) and torch.equal(outs["sparse"].heads[:, 0], ids.n_clusters)

        # what a caller does today, on the first host-maps maps
        host_results = {}
        H = min(args.host_maps, B)
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None and H > 0:
            for name in outs:
                if name == "spirals" or name.endswith("_tile"):
                    continue
                s, kw = calls[name]
                arm = dict(lo=kw.get("lo", 0), hi=kw.get("hi", INT32_MAX), connectivity=8, min_cells=kw.get("min_cells", 1))
                same = bool(torch.equal(host_regions(torch, ndimage, s[:H], **arm), outs[name].cell_cluster[:H]))
                walls = []
                for _ in range(args.host_reps):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    host_regions(torch, ndimage, s[:H], **arm)
                    stream.synchronize()
                    walls.append((time.perf_counter() - t0) * 1e3)
                host_results[name] = {"maps": H, "ms_median_measured": float(np.median(walls)), "ms_scaled_to_all_maps": float(np.median(walls)) * B / H,
                                      "equals_the_call": same}

        per_cell = {"copy_28": 28, "copy_32": 32, "copy_52": 52}
        copies = [c for c in per_cell if c in args.arms]
        if copies:
            words = B * cells * max(per_cell[c] for c in copies) // 8  # (a copy reads half of its traffic and writes half)
            src = torch.zeros(words, dtype=torch.int32, device="cuda")
            dst = torch.empty_like(src)

        def run(what):
            if what in outs:
                s, kw = calls[what]
                seg.debug_regions_tile(1 if what.endswith("_tile") else 0)
                seg.cluster_planes(s, out=outs[what], on_torch_stream=True, **kw)
            elif what == "cluster_plane":
                seg.cluster_clouds(pts, n_pts, labels=batch.labels, out=ids, on_torch_stream=True, **cluster_kw)
            else:
                k = B * cells * per_cell[what] // 8
                dst[:k].copy_(src[:k])

        events = {}
        order = [a for a in ALL_ARMS if a in args.arms]
        for rep in range(-args.warmup, args.reps):
            for what in order:  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(what)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d maps" % B, "host_composition": host_results}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
        if what in per_cell:
            results[what]["GBps"] = B * cells * per_cell[what] / float(np.median(t)) / 1e6
    for arm, copy in (("dense_occ", "copy_28"), ("dense_blocked", "copy_28"), ("sparse", "copy_28"), ("frontier_m1", "copy_32"), ("frontier_m5", "copy_52")):
        for name in (arm, arm + "_tile"):
            if name in results and copy in results:
                results[name]["ratio_over_its_copy"] = results[name]["ms_median"] / results[copy]["ms_median"]
            if name in results and arm in host_results:
                results[name]["ratio_host_over_call"] = host_results[arm]["ms_scaled_to_all_maps"] / results[name]["ms_median"]
    results["regions_tile_default"] = seg.debug_regions_tile()
    if "sparse" in results and "cluster_plane" in results:
        spread = results["cluster_plane"]["ms_max"] - results["cluster_plane"]["ms_min"]
        results["sparse_not_slower_than_cluster_plane_beyond_its_spread"] = bool(results["sparse"]["ms_median"] <= results["cluster_plane"]["ms_median"] + spread)
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
