#!/usr/bin/env python3
"""gg_box_clusters on the headline shape (1024 GG_POINT16 clouds of a 64-ring scan on maps of 364 x 364, ids and counts those of
cluster_clouds behind filter_batch), max_clusters = 256, timed by stream events, median of --reps with the warm-up excluded; ms per 1024
clouds unless said otherwise:

  edge16         (a) K = 16 headings over [0, 90 degrees), GG_BOX_EDGE, records only
  edge16_costs   (b) ... with the d_costs volume
  area16, area16_costs   (c) the same two under GG_BOX_AREA (no second walk)
  edge8, edge32  (d) (a) with K = 8 and K = 32
  single         (e) (a) on ONE cloud: one work-group on one compute unit, a latency
  copy           (f) one device-to-device copy that moves as many bytes as (a)'s algorithmic traffic -- the ids once per slab, 16 bytes per
                 participating point per walk (two walks under EDGE), the records; it reads half of them and writes half: the bandwidth
                 yardstick of this session
  torch          (g) the caller's alternative on the same device, per map and per heading: the two projections as int64, scatter_reduce
                 amin / amax by id, for EDGE a gather of the extrema and a scatter_add.  Timed on --sample maps and scaled to all of them;
                 its records and cost volume are asserted bit-equal to (b)'s before anything is timed

Every repetition runs (a) (f) (a) (f) (b) (c) (d) (e) (g); the two A/B pairs are reported apart.  Needs a GPU; writes one JSON file and
prints it.  For times per kernel run the tool alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_boxes.py --reps 3`.

    python tools/bench_boxes.py --out profiles/boxes/summary.json
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402


def torch_boxes(torch, xy, ids, n_clusters, pos, scale, rot, M, edge):
    """what a caller composes today for ONE map: xy float32 [n, 2] map-frame points, ids int32 [n] (cluster_clouds gives an id >= 0 to
    points inside the map only, so the id alone decides participation), rot int64 [K, 2].  Returns (records int32 [M, 8], costs int64
    [M, K]); rows from min(n_clusters, M) on are not meaningful.  Nothing synchronises."""
    dev = xy.device
    Mi = torch.clamp(n_clusters.long(), 0, M)
    ids = ids.long()
    part = (ids >= 0) & (ids < Mi)
    c = ids[part]
    ux = torch.floor((xy[part, 0].double() - pos[0]) * scale).long()
    uy = torch.floor((xy[part, 1].double() - pos[1]) * scale).long()
    K = rot.shape[0]
    big = torch.iinfo(torch.int64).max
    cnt = torch.zeros(M, dtype=torch.int64, device=dev).index_add_(0, c, torch.ones_like(c))
    cols = {k: [] for k in ("a_min", "a_max", "b_min", "b_max", "cost")}
    for k in range(K):
        cq, sq = rot[k, 0], rot[k, 1]
        a, b = ux * cq + uy * sq, uy * cq - ux * sq
        lo_a = torch.full((M,), big, dtype=torch.int64, device=dev).scatter_reduce(0, c, a, "amin")
        hi_a = torch.full((M,), -big, dtype=torch.int64, device=dev).scatter_reduce(0, c, a, "amax")
        lo_b = torch.full((M,), big, dtype=torch.int64, device=dev).scatter_reduce(0, c, b, "amin")
        hi_b = torch.full((M,), -big, dtype=torch.int64, device=dev).scatter_reduce(0, c, b, "amax")
        if edge:
            d = torch.minimum(torch.minimum(a - lo_a[c], hi_a[c] - a), torch.minimum(b - lo_b[c], hi_b[c] - b))
            cost = torch.zeros(M, dtype=torch.int64, device=dev).index_add_(0, c, d)
        else:
            cost = (hi_a - lo_a) * (hi_b - lo_b)
        for name, v in (("a_min", lo_a), ("a_max", hi_a), ("b_min", lo_b), ("b_max", hi_b), ("cost", cost)):
            cols[name].append(v)
    t = {name: torch.stack(v, 1) for name, v in cols.items()}  # [M, K]
    has = cnt > 0
    costs = torch.where(has[:, None], t["cost"], torch.full_like(t["cost"], -1))
    # the smallest cost, the smallest k among equals: the costs are non-negative int64 (below 2^63), so argmin of (cost, k) in two steps
    least = t["cost"].min(1).values
    kstar = torch.where(t["cost"] == least[:, None], torch.arange(K, device=dev)[None, :], K).min(1).values
    pick = kstar[:, None]
    zero = torch.zeros_like(cnt)
    fields = [torch.where(has, kstar, zero - 1), cnt]
    fields += [torch.where(has, t[name].gather(1, pick)[:, 0], zero) for name in ("a_min", "a_max", "b_min", "b_max")]
    fields += [torch.where(has, least & 0xFFFFFFFF, zero), torch.where(has, least >> 32, zero)]
    rec = torch.stack(fields, 1)
    rec = torch.where(rec >= 2 ** 31, rec - 2 ** 32, rec).to(torch.int32)  # (cost_lo: the int32 with the bits of the low word)
    return rec, costs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--sample", type=int, default=4, help="maps the torch alternative is run on (its time is scaled to --clouds)")
    ap.add_argument("--max-clusters", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_boxes.py needs a GPU")
    B, M, sample = args.clouds, args.max_clusters, min(args.sample, args.clouds)
    base = [synth.hdl64_cloud(seed=3000 + k, n_az=args.n_az) for k in range(16)]
    stride = (max(len(c) for c in base) + 63) // 64 * 64
    host = np.zeros((16, stride), dtype=api.POINT16_DTYPE)
    for k, c in enumerate(base):
        host[k, : len(c)] = api.pack16(c)
    pts = torch.from_numpy(host.view(np.uint8).reshape(16, stride, 16)).cuda().repeat((B + 15) // 16, 1, 1)[:B].contiguous()
    n_pts = [len(base[b % 16]) for b in range(B)]
    origins, base_z = np.zeros((B, 3), np.float32), np.full(B, -1.73)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride)
    tables = {K: api.rotation_table([k * (math.pi / 2) / K for k in range(K)]) for K in (8, 16, 32)}
    variants = {"edge16": (16, "edge", False), "edge16_costs": (16, "edge", True), "area16": (16, "area", False), "area16_costs": (16, "area", True),
                "edge8": (8, "edge", False), "edge32": (32, "edge", False)}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)
        seg.batch_fence()
        cl = seg.cluster_clouds(pts, n_pts, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5, max_clusters=M)
        ids, counts = cl.point_cluster, cl.n_clusters

        def call(name, out=None):
            K, crit, costs = variants[name]
            return seg.box_clusters(pts, n_pts, ids, counts, tables[K], criterion=crit, max_clusters=M, costs=costs, out=out, on_torch_stream=True)

        outs = {name: call(name) for name in variants}
        one = seg.box_clusters(pts[:1], n_pts[:1], ids[:1], counts[:1], tables[16], max_clusters=M, on_torch_stream=True)
        # the alternative, and that it says what the call says
        xy = pts.view(torch.float32).view(B, stride, 4)
        scale = 16.0 / float(np.float32(0.33))
        rot16 = torch.from_numpy(tables[16].astype(np.int64)).cuda()

        def alternative(i, edge):
            return torch_boxes(torch, xy[i, : n_pts[i], :2], ids[i, : n_pts[i]], counts[i], seg.map(i).getPosition(), scale, rot16, M, edge)

        stream.synchronize()
        host_counts = counts.cpu().numpy()
        for name, edge in (("edge16_costs", True), ("area16_costs", False)):
            for i in range(sample):
                rec, costs = alternative(i, edge)
                Mi = min(max(int(host_counts[i]), 0), M)
                assert torch.equal(rec[:Mi], outs[name].boxes[i, :Mi]) and torch.equal(costs[:Mi], outs[name].costs[i, :Mi]), f"{name}: map {i}"
        assert torch.equal(outs["edge16"].boxes[0, : min(max(int(host_counts[0]), 0), M)], one.boxes[0, : min(max(int(host_counts[0]), 0), M)])
        Mi = np.clip(host_counts, 0, M).astype(np.int64)
        boxes = outs["edge16"].boxes.cpu().numpy()
        participating = np.array([int(boxes[i, : Mi[i], 1].sum()) for i in range(B)], dtype=np.int64)
        slabs = {K: -(-Mi // _lib.box_slab_clusters(K, M)) for K in (8, 16, 32)}
        traffic = int((slabs[16] * 4 * np.array(n_pts)).sum() + 2 * 16 * participating.sum() + 32 * Mi.sum())
        src = torch.empty(max(traffic // 8, 1), dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        shape = {"clouds": B, "rows": seg.rows, "cols": seg.cols, "max_clusters": M, "points_per_cloud": float(np.mean(n_pts)),
                 "clusters_of_cluster_clouds_per_cloud": float(host_counts.mean()), "boxed_clusters_per_cloud": float(Mi.mean()),
                 "participating_points_per_cloud": float(participating.mean()), "slabs_per_cloud": {str(K): float(v.mean()) for K, v in slabs.items()},
                 "slab_clusters": {str(K): _lib.box_slab_clusters(K, M) for K in (8, 16, 32)}, "algorithmic_bytes_edge16": traffic,
                 "copy_bytes_read_plus_written": int(src.numel()) * 8, "torch_sample_maps": sample}

        def run(what):
            if what.startswith("copy"):
                dst.copy_(src)
            elif what == "single":
                seg.box_clusters(pts[:1], n_pts[:1], ids[:1], counts[:1], tables[16], max_clusters=M, out=one, on_torch_stream=True)
            elif what == "torch_edge":
                for i in range(sample):
                    alternative(i, True)
            elif what == "torch_area":
                for i in range(sample):
                    alternative(i, False)
            else:
                name = what[:-2] if what[-2:] in ("_1", "_2") else what
                call(name, outs[name])

        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in ("edge16_1", "copy_1", "edge16_2", "copy_2", "edge16_costs", "area16", "area16_costs", "edge8", "edge32", "single", "torch_edge", "torch_area"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(what)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup,
               "unit": "ms per %d clouds (single: per cloud; torch_*: per %d maps, scaled below)" % (B, sample), "torch_equals_the_call_on_the_sample": True}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    a = 0.5 * (results["edge16_1"]["ms_median"] + results["edge16_2"]["ms_median"])
    results["edge16_ms"] = a
    results["ratio_edge16_over_copy"] = [results["edge16_%d" % k]["ms_median"] / results["copy_%d" % k]["ms_median"] for k in (1, 2)]
    for crit, mine in (("edge", a), ("area", results["area16"]["ms_median"])):
        results["torch_%s_ms_scaled_to_all_clouds" % crit] = results["torch_" + crit]["ms_median"] * B / sample
        results["ratio_torch_%s_scaled_over_the_call" % crit] = results["torch_%s_ms_scaled_to_all_clouds" % crit] / mine
    results["edge16_GBps_algorithmic"] = traffic / a / 1e6
    results["copy_GBps"] = [shape["copy_bytes_read_plus_written"] / results["copy_%d" % k]["ms_median"] / 1e6 for k in (1, 2)]
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
