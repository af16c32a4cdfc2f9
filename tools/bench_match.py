#!/usr/bin/env python3
"""gg_match_planes on the headline shape of tools/bench_fusion.py (1024 maps of 364 x 364).  The planes are those of that benchmark's drive:
visibility_clouds on 1024 GG_POINT16 clouds of a 64-ring scan, fused by fuse_states over two frames with a non-zero index shift between
them; the scan is the state plane of the last frame, the field is the evidence of the frames before it, and the prior shift is the one the
third fuse_states call of that benchmark takes.  Window 8 (289 translations) and 21 yaw candidates 0.2 degrees apart around zero, the
identity first.  Timed by stream events, median of --reps with the warm-up excluded; ms per call:

  best            (a) match_planes, d_best alone: 21 yaws
  best_scores     (b) as (a) with the score volumes written
  one_yaw         (c) as (a) with the identity alone
  copy            (d) one device-to-device copy that moves as many bytes as (a)'s algorithmic traffic -- the scan and the field read once, the
                  rows of d_best written (it reads half of them and writes half): the bandwidth yardstick of this session.  The call is no
                  copy: it makes scan cells * yaws * translations look-ups, which is what (a) is divided by
  one_map         (e) as (a) for n = 1: 21 work-groups -- a latency, measured and written down, not a target

  torch           the caller's alternative on the same device, per map: nonzero (which synchronises), and per yaw the rotation in int64 and
                  a scatter-add into a count canvas; the clamped, padded field unfolded once into its (2 W + 1)^2 translations and one
                  matmul of the count canvases with them (float32: every sum is an integer below 2^24, so it is exact); the best by the
                  tie rule from a packed key -- on --sample maps, scaled to all of them.  Its d_best is asserted equal to (a)'s on bits

Every repetition runs (a) (b) (c) (d); (e) runs --reps-slow times behind them.  Needs a GPU; writes one JSON file and prints it.  For
times per kernel run the tool alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_match.py --reps 3`.

    python tools/bench_match.py --out profiles/match/summary.json
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

FUSE = dict(hit=4, miss=1, decay=1, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)  # tools/bench_fusion.py PARAMS
MATCH = dict(window=8, field_max=32)


def torch_match(scan, field, shift, pivot, table, W, field_max, rank):
    """d_best of one map in torch on the device (see the module text); table: int64 [K, 2], rank: int64 [K, D, D] packed tie ranks"""
    import torch
    import torch.nn.functional as F

    rows, cols = scan.shape
    D = 2 * W + 1
    r, c = torch.nonzero(scan > 0, as_tuple=True)
    reward = F.pad(field.clamp(0, field_max).float(), (2 * W, 2 * W, 2 * W, 2 * W))
    shifted = F.unfold(reward[None, None], (rows + 2 * W, cols + 2 * W))[0]  # [canvas cells, D * D]
    dr, dc = r - pivot[0], c - pivot[1]
    counts = torch.zeros((len(table), (rows + 2 * W) * (cols + 2 * W)), dtype=torch.float32, device=scan.device)
    ones = torch.ones(len(r), dtype=torch.float32, device=scan.device)
    for k in range(len(table)):
        cq, sq = table[k, 0], table[k, 1]
        a, b = cq * dr - sq * dc, sq * dr + cq * dc
        u = pivot[0] + torch.sign(a) * ((a.abs() + 8192) >> 14) + shift[0] + W
        v = pivot[1] + torch.sign(b) * ((b.abs() + 8192) >> 14) + shift[1] + W
        ok = (u >= 0) & (u < rows + 2 * W) & (v >= 0) & (v < cols + 2 * W)
        counts[k].index_put_((u[ok] * (cols + 2 * W) + v[ok],), ones[ok], accumulate=True)
    S = (counts @ shifted).round().long().view(len(table), D, D)
    key = (S << 32) | (0xFFFFFFFF - rank)
    at = int(key.argmax().item())
    k, dy, dx = at // (D * D), at // D % D - W, at % D - W
    top = S.view(-1)[at]
    return torch.stack([torch.tensor(v, device=scan.device) for v in (k, dy, dx)] + [top, torch.tensor(len(r), device=scan.device), (S == top).sum()]).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-slow", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--yaws", type=int, default=21)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_match.py needs a GPU")
    B, W, K = args.maps, MATCH["window"], args.yaws
    D = 2 * W + 1
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
    steps = np.concatenate([[0], np.repeat(np.arange(1, K // 2 + 1), 2) * np.tile([1, -1], K // 2)])[:K]  # 0, +1, -1, +2, -2, ...
    table = api.rotation_table(np.radians(0.2 * steps))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        first = seg.fuse_states(states, on_torch_stream=True, **FUSE)
        field = seg.fuse_states(states, first.evidence, shifts=-shifts, on_torch_stream=True, **FUSE).evidence
        del first

        best = seg.match_planes(states, field, shifts=shifts, rotations=table, on_torch_stream=True, **MATCH)
        full = seg.match_planes(states, field, shifts=shifts, rotations=table, scores=True, on_torch_stream=True, **MATCH)
        single = seg.match_planes(states, field, shifts=shifts, on_torch_stream=True, **MATCH)
        one = seg.match_planes(states[:1], field[:1], shifts=shifts[:1], rotations=table, on_torch_stream=True, **MATCH)
        stream.synchronize()
        assert torch.equal(best.best, full.best) and torch.equal(one.best[0], best.best[0])
        assert torch.equal(full.scores.view(B, -1).max(1).values, best.best[:, 3]) and torch.equal(full.scores[:, 0].reshape(B, -1).max(1).values, single.best[:, 3])
        assert torch.equal((states > 0).sum((1, 2)).to(torch.int32), best.best[:, 4])

        # the caller's alternative, on a sample of maps
        sample = sorted({int(i) for i in np.linspace(0, B - 1, min(args.sample, B))})
        table_dev = torch.from_numpy(table.astype(np.int64)).cuda()
        off = torch.arange(-W, W + 1, device="cuda")
        rank = ((off[:, None] ** 2 + off[None, :] ** 2)[None] << 20) | (torch.arange(K, device="cuda")[:, None, None] << 14) | ((off[:, None] + W) << 7)[None] | (off[None, :] + W)[None]
        pivot = (rows // 2, cols // 2)
        torch_match(states[0], field[0], shifts[0].tolist(), pivot, table_dev, W, MATCH["field_max"], rank)  # (warm-up: the first launches)
        t_torch = []
        for i in sample:
            stream.synchronize()
            t0 = time.perf_counter()
            got = torch_match(states[i], field[i], shifts[i].tolist(), pivot, table_dev, W, MATCH["field_max"], rank)
            stream.synchronize()
            t_torch.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(got, best.best[i]), f"map {i}: torch {got.tolist()} and match_planes {best.best[i].tolist()} differ"
        scan_cells = int(best.best[:, 4].long().sum().item())
        traffic = 2 * B * cells * 4 + B * 6 * 4  # the scan and the field read once, the rows written
        src = torch.empty(traffic // 8, dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        b = best.best.double()
        shape = {"maps": B, "rows": rows, "cols": cols, "fuse_params": FUSE, "match_params": MATCH, "yaws": K, "yaw_step_deg": 0.2, "prior_shift": [3, -2],
                 "scan_cells_per_map": scan_cells / B, "positive_field_cells_per_map": float((field > 0).sum().item()) / B,
                 "lookups_best": scan_cells * K * D * D, "lookups_one_yaw": scan_cells * D * D, "lookups_one_map": int(best.best[0, 4].item()) * K * D * D,
                 "best_score_mean": float(b[:, 3].mean().item()), "ties_mean": float(b[:, 5].mean().item()),
                 "maps_corrected_to_zero": int(((best.best[:, :3] == 0).all(1)).sum().item()),
                 "algorithmic_bytes_best": traffic, "algorithmic_bytes_best_scores": traffic + B * K * D * D * 4, "copy_bytes_read_plus_written": int(src.numel()) * 8}

        def run(what):
            if what == "best":
                seg.match_planes(states, field, shifts=shifts, rotations=table, out=best, on_torch_stream=True, **MATCH)
            elif what == "best_scores":
                seg.match_planes(states, field, shifts=shifts, rotations=table, scores=True, out=full, on_torch_stream=True, **MATCH)
            elif what == "one_yaw":
                seg.match_planes(states, field, shifts=shifts, out=single, on_torch_stream=True, **MATCH)
            elif what == "copy":
                dst.copy_(src)
            else:
                seg.match_planes(states[:1], field[:1], shifts=shifts[:1], rotations=table, out=one, on_torch_stream=True, **MATCH)

        events = {}

        def timed(what, keep):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(what)
            e1.record()
            if keep:
                events.setdefault(what, []).append((e0, e1))

        for rep in range(-args.warmup, args.reps):
            for what in ("best", "best_scores", "one_yaw", "copy"):
                timed(what, rep >= 0)
        stream.synchronize()
        for rep in range(-1, args.reps_slow):
            timed("one_map", rep >= 0)
        stream.synchronize()  # (once per group: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "reps_slow": args.reps_slow, "warmup": args.warmup, "unit": "ms per call", "torch_equals_best_on_the_sample": True}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    results["torch"] = {"sample": sample, "ms_per_map": t_torch, "ms_per_map_median": float(np.median(t_torch)), "ms_scaled_to_all_maps": float(np.median(t_torch)) * B}
    results["ratio_torch_over_best"] = results["torch"]["ms_scaled_to_all_maps"] / results["best"]["ms_median"]
    results["ratio_best_over_copy"] = results["best"]["ms_median"] / results["copy"]["ms_median"]
    results["ratio_best_over_one_yaw"] = results["best"]["ms_median"] / results["one_yaw"]["ms_median"]
    results["ratio_best_scores_over_best"] = results["best_scores"]["ms_median"] / results["best"]["ms_median"]
    results["copy_GBps"] = shape["copy_bytes_read_plus_written"] / results["copy"]["ms_median"] / 1e6
    results["best_Glookups_per_s"] = shape["lookups_best"] / results["best"]["ms_median"] / 1e6
    results["one_yaw_Glookups_per_s"] = shape["lookups_one_yaw"] / results["one_yaw"]["ms_median"] / 1e6
    results["one_map_Glookups_per_s"] = shape["lookups_one_map"] / results["one_map"]["ms_median"] / 1e6
    results["best_us_per_map"] = results["best"]["ms_median"] * 1e3 / B
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
