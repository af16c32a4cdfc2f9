#!/usr/bin/env python3
"""gg_footprint_planes on the headline shape of tools/bench_fusion.py (1024 maps of 364 x 364).  The blocked planes are the fused states of
that benchmark's drive: visibility_clouds on 1024 GG_POINT16 clouds of a 64-ring scan, fused by fuse_states over two frames with a
non-zero index shift between them (blocked: occupied or never observed).  The footprint is a car of 4.7 m x 1.9 m on 0.33 m cells with the
reference cell at the rear axle (11.2 cells ahead, 3.0 behind, 2.9 to either side, the default pad) at 32 headings, R = 14, the outside
blocked.  Timed by stream events, median of --reps with the warm-up excluded; ms per call:

  all             (a) footprint_planes, mask + fit + counts
  mask            (b) the mask alone
  one_heading     (c) as (a) with the first heading alone (K = 1)
  radius_32       (d) as (a) with a footprint of 28 x 8 cells ahead, 7 to either side, in a table of R = 32
  one_cell        (d') as (a) with the footprint of one cell, K = 1 and R = 0: no halo, one row -- what reading a plane into bitmaps and
                  writing two planes costs
  copy            (e) one device-to-device copy that moves as many bytes as (a)'s algorithmic traffic -- 4 bytes read and 4 written per given
                  plane, per cell (it reads half of them and writes half): the bandwidth yardstick of this session
  one_map         (f) as (a) for n = 1: 36 work-groups -- a latency, measured and written down, not a target

  torch           the caller's alternative on the same device, per map: the blocked plane as float, padded by R with ones, conv2d with the
                  K footprint kernels of (2 R + 1)^2 (every sum is an integer below 2^24, so float32 is exact), == 0, the K planes packed
                  into one mask word -- on --sample maps, scaled to all of them.  Its mask is asserted equal to (a)'s on bits

Every repetition runs (a) (b) (c) (d) (d') (e); (f) runs --reps-slow times behind them.  Needs a GPU; writes one JSON file and prints it.  For
times per kernel run the tool alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_footprint.py --reps 3`.

    python tools/bench_footprint.py --out profiles/footprint/summary.json
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

# tools/bench_fusion.py PARAMS, but without decay: with decay 1 and miss 1 two frames leave no cell free, and nothing would fit anywhere
FUSE = dict(hit=4, miss=1, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)
CAR = dict(ahead=11.2, behind=3.0, left=2.9, right=2.9)
LARGE = dict(ahead=28.0, behind=8.0, left=7.0, right=7.0)


def footprint_kernels(spans, device):
    """float32 [K, 1, 2 R + 1, 2 R + 1]: 1 on the cells of every heading"""
    import torch

    K, R = spans.shape[0], spans.shape[1] // 2
    kernels = torch.zeros((K, 1, 2 * R + 1, 2 * R + 1), dtype=torch.float32, device=device)
    for k in range(K):
        for a in range(2 * R + 1):
            lo, hi = int(spans[k, a, 0]), int(spans[k, a, 1])
            if lo <= hi:
                kernels[k, 0, a, lo + R: hi + R + 1] = 1.0
    return kernels


def torch_footprint(blocked, kernels, outside_free):
    """the mask of one map in torch (see the module text): int64 [rows, cols] holding the 32 bits of the word"""
    import torch
    import torch.nn.functional as F

    K, R = kernels.shape[0], kernels.shape[2] // 2
    taken = F.pad((blocked >= 0).float()[None, None], (R, R, R, R), value=0.0 if outside_free else 1.0)
    fits = F.conv2d(taken, kernels)[0] == 0  # (cross-correlation: the footprint laid over the map, not reflected)
    return (fits.long() << torch.arange(K, device=blocked.device)[:, None, None]).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-slow", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--headings", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_footprint.py needs a GPU")
    B, K = args.maps, args.headings
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
    table = api.rotation_table(2.0 * np.pi * np.arange(K) / K)
    car = api.footprint_spans(table, **CAR, radius=14)
    large = api.footprint_spans(table, **LARGE, radius=32)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        first = seg.fuse_states(states, on_torch_stream=True, **FUSE)
        blocked = seg.fuse_states(states, first.evidence, shifts=-shifts, on_torch_stream=True, **FUSE).state
        del first

        every = seg.footprint_planes(blocked, car, min_fit=1, on_torch_stream=True)
        alone = seg.footprint_planes(blocked, car, min_fit=1, fit=False, counts=False, on_torch_stream=True)
        single = seg.footprint_planes(blocked, car[:1], min_fit=1, on_torch_stream=True)
        wide = seg.footprint_planes(blocked, large, min_fit=1, on_torch_stream=True)
        point = seg.footprint_planes(blocked, np.zeros((1, 1, 2), np.int32), min_fit=1, on_torch_stream=True)
        one = seg.footprint_planes(blocked[:1], car, min_fit=1, on_torch_stream=True)
        stream.synchronize()
        assert torch.equal(every.mask, alone.mask) and torch.equal(one.mask[0], every.mask[0]) and torch.equal(one.counts[0], every.counts[0])
        assert torch.equal(single.mask, every.mask & 1) and torch.equal(point.mask, (blocked < 0).to(torch.int32))
        assert torch.equal((every.fit == -1).sum((1, 2)).to(torch.int32), every.counts[:, 1]) and torch.equal((every.mask == 0).sum((1, 2)).to(torch.int32), every.counts[:, 2])

        # the caller's alternative, on a sample of maps
        sample = sorted({int(i) for i in np.linspace(0, B - 1, min(args.sample, B))})
        kernels = footprint_kernels(car, "cuda")
        torch_footprint(blocked[0], kernels, False)  # (warm-up: the first launches, the choice of a convolution algorithm)
        t_torch = []
        for i in sample:
            stream.synchronize()
            t0 = time.perf_counter()
            got = torch_footprint(blocked[i], kernels, False)
            stream.synchronize()
            t_torch.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(got, every.mask[i].long() & 0xFFFFFFFF), f"map {i}: the torch mask and footprint_planes differ"
        traffic = B * cells * 4 * 3  # the blocked plane read once, the mask and the fit plane written (the counts are 12 bytes per map)
        src = torch.empty(traffic // 8, dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        c = every.counts.double()
        footprint_cells = [int(np.maximum(t[..., 1] - t[..., 0] + 1, 0).sum()) for t in (car, large)]
        shape = {"maps": B, "rows": rows, "cols": cols, "fuse_params": FUSE, "headings": K, "car": CAR, "car_radius": 14, "large": LARGE, "large_radius": 32,
                 "min_fit": 1, "outside_free": 0, "blocked_cells_per_map": float((blocked >= 0).sum().item()) / B,
                 "cells_every_heading_fits_per_map": float(c[:, 0].mean().item()), "cells_some_heading_fits_per_map": float(c[:, 1].mean().item()),
                 "cells_no_heading_fits_per_map": float(c[:, 2].mean().item()), "footprint_cells_car_all_headings": footprint_cells[0],
                 "footprint_cells_large_all_headings": footprint_cells[1], "lookups_of_the_direct_form_all": B * cells * footprint_cells[0],
                 "algorithmic_bytes_all": traffic, "algorithmic_bytes_mask": B * cells * 4 * 2, "copy_bytes_read_plus_written": int(src.numel()) * 8}

        def run(what):
            if what == "all":
                seg.footprint_planes(blocked, car, min_fit=1, out=every, on_torch_stream=True)
            elif what == "mask":
                seg.footprint_planes(blocked, car, min_fit=1, fit=False, counts=False, out=alone, on_torch_stream=True)
            elif what == "one_heading":
                seg.footprint_planes(blocked, car[:1], min_fit=1, out=single, on_torch_stream=True)
            elif what == "radius_32":
                seg.footprint_planes(blocked, large, min_fit=1, out=wide, on_torch_stream=True)
            elif what == "one_cell":
                seg.footprint_planes(blocked, np.zeros((1, 1, 2), np.int32), min_fit=1, out=point, on_torch_stream=True)
            elif what == "copy":
                dst.copy_(src)
            else:
                seg.footprint_planes(blocked[:1], car, min_fit=1, out=one, on_torch_stream=True)

        events = {}

        def timed(what, keep):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(what)
            e1.record()
            if keep:
                events.setdefault(what, []).append((e0, e1))

        for rep in range(-args.warmup, args.reps):
            for what in ("all", "mask", "one_heading", "radius_32", "one_cell", "copy"):
                timed(what, rep >= 0)
        stream.synchronize()
        for rep in range(-1, args.reps_slow):
            timed("one_map", rep >= 0)
        stream.synchronize()  # (once per group: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "reps_slow": args.reps_slow, "warmup": args.warmup, "unit": "ms per call", "torch_equals_mask_on_the_sample": True}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    results["torch"] = {"sample": sample, "ms_per_map": t_torch, "ms_per_map_median": float(np.median(t_torch)), "ms_scaled_to_all_maps": float(np.median(t_torch)) * B}
    results["ratio_torch_over_all"] = results["torch"]["ms_scaled_to_all_maps"] / results["all"]["ms_median"]
    results["ratio_all_over_copy"] = results["all"]["ms_median"] / results["copy"]["ms_median"]
    results["ratio_all_over_one_heading"] = results["all"]["ms_median"] / results["one_heading"]["ms_median"]
    results["ratio_radius_32_over_all"] = results["radius_32"]["ms_median"] / results["all"]["ms_median"]
    results["copy_GBps"] = shape["copy_bytes_read_plus_written"] / results["copy"]["ms_median"] / 1e6
    results["all_algorithmic_GBps"] = shape["algorithmic_bytes_all"] / results["all"]["ms_median"] / 1e6
    results["all_G_direct_lookups_per_s"] = shape["lookups_of_the_direct_form_all"] / results["all"]["ms_median"] / 1e6
    results["all_us_per_map"] = results["all"]["ms_median"] * 1e3 / B
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
