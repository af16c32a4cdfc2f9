#!/usr/bin/env python3
"""gg_export_images on the headline shape (1024 maps of 364 x 364 after one default batch), timed by stream events, median of --reps with
the warm-up excluded, the variants alternating inside every repetition:

  (a) gg_export_images, the tiled kernels ("images_variant" 0): one layer (ground), all eleven layers, the terrain image alone
  (b) the same through the cell-by-cell kernels ("images_variant" 1)
  (c) gg_export_layers of the same mask on the same maps, row-major: the floor for reading the sources once (the u8 path reads them
      twice and writes a quarter of the bytes).  For the terrain image: the export of ground + pointsRaw, the two layers it reads.
  (d) the loop of the single-map getters (gg_get_layer_image_u8 / gg_get_terrain_image) over --getter-slots maps by the wall clock,
      scaled to all maps: what a caller had before.

and the ratios (a)/(c) and (d)/(a).  Needs a GPU; writes one JSON file and prints it.

    python tools/bench_images.py --out profiles/images/summary.json
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
from groundgrid_amd._lib import LAYERS  # noqa: E402

# case -> (u8 layers, terrain, the layers of the export that reads the same sources once)
CASES = {"one_layer": (["ground"], False, ["ground"]), "all_eleven": (list(LAYERS), False, list(LAYERS)), "terrain_only": ([], True, ["ground", "pointsRaw"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--getter-slots", type=int, default=64, help="maps of the host loop of single getters")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_images.py needs a GPU")
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
    cells = seg.rows * seg.cols
    stream = torch.cuda.Stream()
    shipped = seg.debug_set_tuning("images_variant_default", 0)
    results = {"shape": {"maps": B, "rows": seg.rows, "cols": seg.cols, "points_per_cloud": int(np.mean(n_pts))}, "reps": args.reps, "warmup": args.warmup,
               "shipped_variant": "cell_by_cell" if shipped else "tiled", "cases": {}}
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        planes = torch.empty((B * len(LAYERS) * cells,), dtype=torch.float32, device="cuda")
        for case, (names, terrain, floor_names) in CASES.items():
            K, Kf = len(names), len(floor_names)
            res = None
            o = planes[: B * Kf * cells].view(B, Kf, seg.rows, seg.cols)
            events = {}
            for rep in range(-args.warmup, args.reps):
                for what in ("a_tiled", "b_cell_by_cell", "c_export_layers"):  # (alternating: all see the same neighbours on the machine)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    if what != "c_export_layers":
                        seg.debug_set_tuning("images_variant", 0 if what == "a_tiled" else 1)
                    e0.record()
                    if what == "c_export_layers":
                        seg.export_layers(floor_names, out=o, row_major=True)
                    else:
                        res = seg.export_images(names, terrain=terrain, out=res, on_torch_stream=True)
                    e1.record()
                    if rep >= 0:
                        events.setdefault(what, []).append((e0, e1))
            stream.synchronize()  # (once per case: the device never idles between repetitions)
            seg.debug_set_tuning("images_variant", shipped)
            entry = {"u8_layers": K, "terrain": terrain, "floor_layers": floor_names,
                     "bytes_written": B * cells * (K + (12 if terrain else 0)), "bytes_written_by_the_floor": B * cells * 4 * Kf}
            for what, ev in events.items():
                t = np.array([a.elapsed_time(b) for a, b in ev])
                entry[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
            a_ms, b_ms, c_ms = (entry[k]["ms_median"] for k in ("a_tiled", "b_cell_by_cell", "c_export_layers"))
            entry["ratio_a_over_c"] = a_ms / c_ms
            entry["ratio_b_over_a"] = b_ms / a_ms
            results["cases"][case] = entry
            del res
    stream.synchronize()
    # (d) what a caller had before: the single-map getters, one synchronous call per map and layer
    n_get = min(args.getter_slots, B)
    for case, (names, terrain, _) in CASES.items():
        def loop(slots):
            for s in slots:
                for k in names:
                    seg.map(s).image_u8(k)
                if terrain:
                    seg.map(s).terrain_image()
        loop(range(min(4, n_get)))
        t0 = time.perf_counter()
        loop(range(n_get))
        wall = (time.perf_counter() - t0) * 1e3
        entry = results["cases"][case]
        shipped_ms = entry["b_cell_by_cell" if shipped else "a_tiled"]["ms_median"]
        entry["d_getter_loop"] = {"maps": n_get, "ms_wall": wall, "ms_scaled_to_all_maps": wall * B / n_get}
        entry["ratio_d_over_a"] = wall * B / n_get / entry["a_tiled"]["ms_median"]
        entry["ratio_d_over_shipped"] = wall * B / n_get / shipped_ms
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
