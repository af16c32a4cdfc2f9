#!/usr/bin/env python3
"""gg_export_slopes on the headline shape (1024 maps of 364 x 364 behind one default batch of the headline clouds), timed by stream events,
median of --reps with the warm-up excluded, the arms alternating inside every repetition; ms per 1024 maps:

  (a) the call with all six channels
  (b) the call with tangent and step only
  (c) the floor: one device-to-device copy of (a)'s algorithmic bytes -- 8 B read per cell plus 4 B written per cell and channel
  (d) gg_debug_set_tuning "slopes_variant" = 1 (cell by cell, nine gathered pairs per cell) on (a)
  (e) what callers do today for the same six planes: export_layers(ground, groundpatch), then torch -- clamped neighbours by
      index_select, subtraction, division, fmax over the eight neighbours, fmin over the nine

and the ratios (a)/(c), (d)/(a), (e)/(a).  (e)'s planes are compared with (a)'s on bits outside NaN cells; the comparison is asserted once,
after the numbers have been written.  Needs a GPU; writes one JSON file and prints it.

    python tools/bench_slopes.py --out profiles/slopes/summary.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api, synth  # noqa: E402

ARMS = ("a_six_channels", "b_tangent_and_step", "c_copy_floor", "d_cell_by_cell", "e_export_and_torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_slopes.py needs a GPU")
    B = args.maps
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
    rows, cols, cells = seg.rows, seg.cols, seg.rows * seg.cols
    res32 = float(np.float32(seg.resolution))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        six = seg.export_slopes(row_major=True)  # (the first call allocates)
        two = seg.export_slopes(["tangent", "step"], row_major=True)
        gathered = torch.empty_like(six)
        layers = seg.export_layers(["ground", "groundpatch"], row_major=True)
        composed = torch.empty_like(six)
        dev = six.device
        r, c = torch.arange(rows, device=dev), torch.arange(cols, device=dev)
        r_lo, r_hi, c_lo, c_hi = (r - 1).clamp(min=0), (r + 1).clamp(max=rows - 1), (c - 1).clamp(min=0), (c + 1).clamp(max=cols - 1)
        den_r = ((r_hi - r_lo).to(torch.float32) * torch.tensor(res32, dtype=torch.float32, device=dev)).view(1, rows, 1)
        den_c = ((c_hi - c_lo).to(torch.float32) * torch.tensor(res32, dtype=torch.float32, device=dev)).view(1, 1, cols)

        one = torch.ones((), dtype=torch.float32, device=dev)

        def torch_arm():
            """what a caller writes today: which way rows and columns run, the border and the fresh-map values are the caller's to restate"""
            seg.export_layers(["ground", "groundpatch"], row_major=True, out=layers)
            g, w = layers[:, 0], layers[:, 1]
            gx = (g.index_select(1, r_lo) - g.index_select(1, r_hi)) / den_r
            gy = (g.index_select(2, c_lo) - g.index_select(2, c_hi)) / den_c
            s = gx * gx
            s += gy * gy
            composed[:, 0], composed[:, 1] = gx, gy
            torch.sqrt(s, out=composed[:, 2])
            torch.div(one, torch.sqrt(s + 1.0), out=composed[:, 3])  # (a division, not a reciprocal kernel)
            step, low = torch.zeros_like(g), w.clone()
            for rr in (r_lo, r, r_hi):
                gr, wr = g.index_select(1, rr), w.index_select(1, rr)
                for cc in (c_lo, c, c_hi):
                    if rr is r and cc is c:
                        continue
                    step = torch.fmax(step, (gr.index_select(2, cc) - g).abs())
                    low = torch.fmin(low, wr.index_select(2, cc))
            composed[:, 4], composed[:, 5] = step, low

        def cell_by_cell():
            seg.debug_set_tuning("slopes_variant", 1)
            seg.export_slopes(row_major=True, out=gathered)
            seg.debug_set_tuning("slopes_variant", 0)

        torch_arm()
        cell_by_cell()
        stream.synchronize()
        a_bits, e_bits, d_bits = six.view(torch.int32), composed.view(torch.int32), gathered.view(torch.int32)
        nan = torch.isnan(six)
        e_equals_a = [bool(((a_bits[:, k] == e_bits[:, k]) | (nan[:, k] & torch.isnan(composed[:, k]))).all().item()) for k in range(6)]
        d_equals_a = bool(torch.equal(a_bits, d_bits))
        nan_cells = int(nan.sum().item())
        floor_bytes = B * cells * (8 + 4 * 6)
        src = torch.empty((floor_bytes // 2,), dtype=torch.uint8, device="cuda")  # a copy of N bytes reads N / 2 and writes N / 2
        dst = torch.empty_like(src)
        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in ARMS:  # (alternating: all see the same neighbours on the machine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if what == "a_six_channels":
                    seg.export_slopes(row_major=True, out=six)
                elif what == "b_tangent_and_step":
                    seg.export_slopes(["tangent", "step"], row_major=True, out=two)
                elif what == "c_copy_floor":
                    dst.copy_(src)
                elif what == "d_cell_by_cell":
                    cell_by_cell()
                else:
                    torch_arm()
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": {"maps": B, "rows": rows, "cols": cols, "order": "row-major", "points_per_cloud_of_the_batch": int(np.mean(n_pts)), "nan_cells_of_a": nan_cells},
               "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d maps" % B, "algorithmic_bytes_of_a": floor_bytes,
               "e_equals_a_outside_nan": dict(zip(_lib.SLOPE_CHANNELS, e_equals_a)), "d_equals_a": d_equals_a}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    a_ms = results["a_six_channels"]["ms_median"]
    results["ratio_a_over_c"] = a_ms / results["c_copy_floor"]["ms_median"]
    results["ratio_d_over_a"] = results["d_cell_by_cell"]["ms_median"] / a_ms
    results["ratio_e_over_a"] = results["e_export_and_torch"]["ms_median"] / a_ms
    results["ratio_b_over_a"] = results["b_tangent_and_step"]["ms_median"] / a_ms
    results["a_effective_GBps"] = floor_bytes / (a_ms * 1e-3) / 1e9
    results["not_measured"] = ["column-major planes", "geometries other than 364 x 364", "contexts of fewer maps", "fresh maps", "per-kernel counters (LDS bank conflicts, fetch size)"]
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    assert all(e_equals_a), "the torch composition and gg_export_slopes differ outside NaN cells: %r" % (results["e_equals_a_outside_nan"],)
    assert d_equals_a, "the cell-by-cell form and the tiled kernel differ"


if __name__ == "__main__":
    main()
