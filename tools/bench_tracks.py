#!/usr/bin/env python3
"""gg_track_clusters on the headline shape (1024 maps of 364 x 364; the id planes those of cluster_clouds on two consecutive frames of 1024
GG_POINT16 clouds of a 64-ring scan, with a move_maps between them whose shifts the call is given), max_clusters = 256, gate = 1, timed by
stream events, median of --reps with the warm-up excluded; ms per 1024 maps unless said otherwise:

  plane          (a) track_clusters with the d_cell_track plane
  no_plane       (b) ... without it
  gate0, gate4   (c) (a) at gate 0 and at gate 4
  single         (d) (a) on ONE map: one work-group on one compute unit, a latency
  copy           (e) one device-to-device copy that moves as many bytes as (a)'s algorithmic traffic (two planes read, one written; it
                 reads half of them and writes half): the bandwidth yardstick of this session
  torch          (f) the caller's alternative on the same device, per map: nonzero, the key c * M + p per offset, a bincount per offset,
                 the maxima by packed keys, a cumulative sum for the ranks.  Timed on --sample maps and scaled to all of them; its records,
                 heads and track plane are asserted bit-equal to (a)'s before anything is timed
  dense          (g) an adversarial scene: 50 % occupancy cut into 2116 clusters of 8 x 8 cells, max_clusters = 1024, so that 1024 x 1024
                 pairs are held 28 rows at a time and the plane is walked once per slab

Every repetition runs (a) (e) (a) (e) (b) (c) (d) (f) (g); the two A/B pairs are reported apart.  Needs a GPU; writes one JSON file and
prints it.  For times per kernel run the tool alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_tracks.py --reps 3`.

    python tools/bench_tracks.py --out profiles/tracks/summary.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import api, synth  # noqa: E402

POSE = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


def torch_tracks(torch, cur, prev, tracks_in, heads_in, shift, M, g):
    """what a caller composes today for ONE map (row-major planes [rows, cols], |shift| < side); returns (records int32 [M, 8] -- the rows
    from heads[1] on are not meaningful --, heads int32 [4], cell_track int32 [rows, cols]).  Nothing synchronises."""
    R, Cc = cur.shape
    s0, s1 = int(shift[0]), int(shift[1])
    dev = cur.device
    valid = (cur >= 0) & (cur < M)
    r, q = torch.nonzero(valid, as_tuple=True)
    c = cur[r, q].long()
    Kc = torch.clamp(cur.max().long() + 1, 0, M)
    Kp = torch.clamp(heads_in[1].long(), 0, M)
    next_id = heads_in[0].long()
    O = torch.zeros(M * M, dtype=torch.int64, device=dev)
    S = O
    for a in range(-g, g + 1):
        for b in range(-g, g + 1):
            rr, qq = r + (s0 + a), q + (s1 + b)
            ok = (rr >= 0) & (rr < R) & (qq >= 0) & (qq < Cc)
            p = prev[rr.clamp(0, R - 1), qq.clamp(0, Cc - 1)].long()
            ok &= (p >= 0) & (p < Kp)
            hist = torch.bincount((c * M + p)[ok], minlength=M * M)
            O = O + hist
            if a == 0 and b == 0:
                S = hist
    O, S = O.view(M, M), S.view(M, M)
    ar = torch.arange(M, device=dev)
    best = (O * M + (M - 1 - ar)[None, :]).max(1).values  # per c: the largest O, among equals the smallest p
    o_c, pstar = best // M, M - 1 - best % M
    has = o_c > 0
    key = torch.where(has, o_c * M + (M - 1 - ar), torch.full_like(o_c, -1))  # per c: its claim on p*(c), among equals the smallest c
    win = torch.full((M,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, pstar, key, "amax")
    inherits = has & (win[pstar] == key)
    born = (ar < Kc) & ~inherits
    rank = torch.cumsum(born.long(), 0) - 1
    tin = tracks_in.long()
    zero = torch.zeros_like(o_c)
    tid = torch.where(inherits, tin[pstar, 0], (next_id + rank) & 0x7FFFFFFF)
    age = torch.where(inherits, tin[pstar, 1].clamp(max=2 ** 31 - 2) + 1, zero)
    ones = torch.ones_like(c)
    cells = torch.zeros(M, dtype=torch.int64, device=dev).index_add_(0, c, ones)
    sum_r = torch.zeros(M, dtype=torch.int64, device=dev).index_add_(0, c, r)
    sum_c = torch.zeros(M, dtype=torch.int64, device=dev).index_add_(0, c, q)
    rec = torch.stack([tid, age, torch.where(inherits, pstar, zero - 1), torch.where(inherits, o_c, zero), torch.where(inherits, S[ar, pstar], zero),
                       cells, sum_r, sum_c], 1).to(torch.int32)
    n_born = born.sum()
    heads = torch.stack([(next_id + n_born) & 0x7FFFFFFF, Kc, n_born, Kp - inherits.sum()]).to(torch.int32)
    cell_track = torch.where(valid, tid[cur.clamp(0, M - 1).long()], torch.full_like(cur, -1, dtype=torch.int64)).to(torch.int32)
    return rec, heads, cell_track


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--sample", type=int, default=8, help="maps the torch alternative is run on (its time is scaled to --maps)")
    ap.add_argument("--max-clusters", type=int, default=256)
    ap.add_argument("--gate", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_tracks.py needs a GPU")
    B, M, g, sample = args.maps, args.max_clusters, args.gate, min(args.sample, args.maps)
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
    moves = np.array([[1.1, -0.8], [-0.5, 0.7], [0.4, 0.4], [-1.4, -0.2]])[np.arange(B) % 4]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        planes = []
        for f in range(2):
            shifts = np.array(seg.move_maps(moves * f, [POSE] * B, on_torch_stream=True), np.int32)
            batch = seg.filter_batch(pts, n_pts, origins, base_z)
            seg.batch_fence()
            cl = seg.cluster_clouds(pts, n_pts, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5, max_clusters=M, point_clusters=False)
            planes.append(cl.cell_cluster.clone())
            n_clusters = cl.n_clusters.double()
        first = seg.track_clusters(planes[0], max_clusters=M, gate=g, on_torch_stream=True)
        full = seg.track_clusters(planes[1], first, shifts, M, g, True, on_torch_stream=True)
        bare = seg.track_clusters(planes[1], first, shifts, M, g, False, on_torch_stream=True)
        gate0 = seg.track_clusters(planes[1], first, shifts, M, 0, True, on_torch_stream=True)
        gate4 = seg.track_clusters(planes[1], first, shifts, M, 4, True, on_torch_stream=True)
        one_prev = api.TrackOutputs(tracks=first.tracks[:1], heads=first.heads[:1], cell_cluster=planes[0][:1])
        one = seg.track_clusters(planes[1][:1], one_prev, shifts[:1], M, g, True, on_torch_stream=True)
        # the alternative, and that it says what the call says
        alt = [torch_tracks(torch, planes[1][i], planes[0][i], first.tracks[i], first.heads[i], shifts[i], M, g) for i in range(sample)]
        stream.synchronize()
        heads = full.heads.cpu().numpy()
        for i, (rec, hd, plane) in enumerate(alt):
            Kc = int(heads[i, 1])
            assert torch.equal(hd, full.heads[i]) and torch.equal(rec[:Kc], full.tracks[i, :Kc]) and torch.equal(plane, full.cell_track[i]), f"map {i}"
        assert torch.equal(bare.heads, full.heads) and torch.equal(one.heads[0], full.heads[0]) and torch.equal(one.cell_track[0], full.cell_track[0])
        del alt
        # the adversarial scene: every second cell occupied, ids by 8 x 8 tile (46 x 46 = 2116 of them), max_clusters = 1024
        tiles = (torch.arange(rows, device="cuda")[:, None] // 8) * ((cols + 7) // 8) + torch.arange(cols, device="cuda")[None, :] // 8
        gen = torch.Generator(device="cuda").manual_seed(23)
        dense_planes = []
        for _ in range(2):
            occ = torch.rand((B, rows, cols), device="cuda", generator=gen) < 0.5
            dense_planes.append(torch.where(occ, tiles[None].to(torch.int32), -1).to(torch.int32).contiguous())
            del occ
        dense_first = seg.track_clusters(dense_planes[0], max_clusters=1024, gate=g, on_torch_stream=True)
        dense = seg.track_clusters(dense_planes[1], dense_first, shifts, 1024, g, True, on_torch_stream=True)
        stream.synchronize()
        h = heads.astype(np.float64)
        dh = dense.heads.cpu().numpy().astype(np.float64)
        traffic = B * rows * cols * 4 * 3  # per cell: this scan's id and the last scan's read, the track id written
        src = torch.empty(traffic // 8, dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        shape = {"maps": B, "rows": rows, "cols": cols, "max_clusters": M, "gate": g, "clusters_of_cluster_clouds_per_map": float(n_clusters.mean().item()),
                 "tracked_clusters_per_map": float(h[:, 1].mean()), "born_per_map": float(h[:, 2].mean()), "ended_per_map": float(h[:, 3].mean()),
                 "cluster_cells_per_map": float((planes[1] >= 0).sum().item()) / B, "largest_shift": int(np.abs(shifts).max()),
                 "algorithmic_bytes_plane": traffic, "copy_bytes_read_plus_written": int(src.numel()) * 8, "torch_sample_maps": sample,
                 "dense": {"max_clusters": 1024, "clusters_per_map": float(dh[:, 1].mean()), "born_per_map": float(dh[:, 2].mean()),
                           "slab_rows": 28 * 1024 // 1024, "slabs": -(-1024 // 28)}}

        def run(what):
            if what.startswith("plane"):
                seg.track_clusters(planes[1], first, shifts, M, g, True, out=full, on_torch_stream=True)
            elif what.startswith("copy"):
                dst.copy_(src)
            elif what == "no_plane":
                seg.track_clusters(planes[1], first, shifts, M, g, False, out=bare, on_torch_stream=True)
            elif what == "gate0":
                seg.track_clusters(planes[1], first, shifts, M, 0, True, out=gate0, on_torch_stream=True)
            elif what == "gate4":
                seg.track_clusters(planes[1], first, shifts, M, 4, True, out=gate4, on_torch_stream=True)
            elif what == "single":
                seg.track_clusters(planes[1][:1], one_prev, shifts[:1], M, g, True, out=one, on_torch_stream=True)
            elif what == "torch":
                for i in range(sample):
                    torch_tracks(torch, planes[1][i], planes[0][i], first.tracks[i], first.heads[i], shifts[i], M, g)
            else:
                seg.track_clusters(dense_planes[1], dense_first, shifts, 1024, g, True, out=dense, on_torch_stream=True)

        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in ("plane_1", "copy_1", "plane_2", "copy_2", "no_plane", "gate0", "gate4", "single", "torch", "dense"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(what)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d maps (single: per map; torch: per %d maps, scaled below)" % (B, sample),
               "torch_equals_plane_on_the_sample": True}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    a = 0.5 * (results["plane_1"]["ms_median"] + results["plane_2"]["ms_median"])
    results["plane_ms"] = a
    results["ratio_plane_over_copy"] = [results["plane_%d" % k]["ms_median"] / results["copy_%d" % k]["ms_median"] for k in (1, 2)]
    results["torch_ms_scaled_to_all_maps"] = results["torch"]["ms_median"] * B / sample
    results["ratio_torch_scaled_over_plane"] = results["torch_ms_scaled_to_all_maps"] / a
    results["ratio_dense_over_plane"] = results["dense"]["ms_median"] / a
    results["plane_GBps_algorithmic"] = traffic / a / 1e6
    results["copy_GBps"] = [shape["copy_bytes_read_plus_written"] / results["copy_%d" % k]["ms_median"] / 1e6 for k in (1, 2)]
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
