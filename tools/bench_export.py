#!/usr/bin/env python3
"""gg_export_layers on the headline shape (1024 maps of 364 x 364 after one default batch): the tiled kernel against the
destination-ordered gather (gg_debug_set_tuning "export_variant"), both plane orders, timed by stream events, and the host loop of
gg_get_layers over the same slots (what a caller had before) by the wall clock.

  (a) ground   (b) ground + groundpatch   (c) all eleven, nothing pending   (d) all eleven, the three lazily kept layers pending

Bytes are what the call has to move, from the shapes: 8 per cell for the interleaved pairs when ground or groundpatch is asked for, 4 per
cell and per-call layer read (an upper bound: only live half columns are read), 4 per cell and plane written.  The share of the copy
ceiling is those bytes over the time over 6.29 TB/s.  Needs a GPU; writes one JSON file and prints it.

    python tools/bench_export.py --out profiles/export_layers/export_layers.json
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

COPY_CEILING_TBS = 6.29
CASES = {"a_ground": ["ground"], "b_ground_groundpatch": ["ground", "groundpatch"], "c_all_eleven": list(LAYERS), "d_all_eleven_lazy_pending": list(LAYERS)}


def nominal_bytes(names, n_maps, cells):
    gp = 8 if ("ground" in names or "groundpatch" in names) else 0
    percall = sum(1 for k in names if k not in ("ground", "groundpatch"))
    return n_maps * cells * (gp + 4 * percall + 4 * len(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--getter-slots", type=int, default=0, help="slots of the host loop (0 = all)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_export.py needs a GPU")
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
    results = {"shape": {"maps": B, "rows": seg.rows, "cols": seg.cols, "points_per_cloud": int(np.mean(n_pts))}, "reps": args.reps,
               "copy_ceiling_TBs": COPY_CEILING_TBS, "cases": {}}
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        out = seg.filter_batch(pts, n_pts, origins, base_z)
        out = seg.filter_batch(pts, n_pts, origins, base_z, out=out)  # (warm maps)
        dst = torch.empty((B, len(LAYERS), seg.cols, seg.rows), dtype=torch.float32, device="cuda")
        flat = dst.view(-1)
        for case, names in CASES.items():
            pending = case.startswith("d_")
            K = len(names)
            shape_c, shape_r = (B, K, seg.cols, seg.rows), (B, K, seg.rows, seg.cols)
            events = {}
            for rep in range(-args.warmup, args.reps):
                for row_major in (False, True):
                    for variant in (0, 1):  # (alternating: both see the same neighbours on the machine)
                        seg.debug_set_tuning("export_variant", variant)
                        if pending:
                            out = seg.filter_batch(pts, n_pts, origins, base_z, out=out)  # (leaves the three layers pending again)
                        o = flat[: B * K * cells].view(shape_r if row_major else shape_c)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        seg.export_layers(names, out=o, row_major=row_major)
                        e1.record()
                        if rep >= 0:
                            events.setdefault((variant, row_major), []).append((e0, e1))
            stream.synchronize()  # (once per case: the device never idles between repetitions)
            times = {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}
            seg.debug_set_tuning("export_variant", seg.debug_set_tuning("export_variant_default", 0))
            nb = nominal_bytes(names, B, cells)
            entry = {"layers": K, "bytes_nominal": nb, "runs": {}}
            for (variant, row_major), t in sorted(times.items()):
                t = np.array(t)
                med = float(np.median(t))
                entry["runs"][f"{'gather' if variant else 'tiled'}_{'rowmajor' if row_major else 'colmajor'}"] = {
                    "ms_median": med, "ms_min": float(t.min()), "ms_max": float(t.max()), "spread_ms": float(t.max() - t.min()),
                    "TBs": nb / (med * 1e-3) / 1e12, "share_of_copy_ceiling": nb / (med * 1e-3) / 1e12 / COPY_CEILING_TBS}
            results["cases"][case] = entry
    stream.synchronize()
    # (e) what a caller had before: one gg_get_layers per slot, on the host
    n_get = args.getter_slots or B
    for s in range(min(8, n_get)):
        seg.map(s).layers()
    t0 = time.perf_counter()
    for s in range(n_get):
        seg.map(s).layers()
    wall = (time.perf_counter() - t0) * 1e3
    per_1024 = wall * B / n_get
    shipped = "gather" if seg.debug_set_tuning("export_variant_default", 0) else "tiled"
    results["shipped_variant"] = shipped
    c_ms = results["cases"]["c_all_eleven"]["runs"][f"{shipped}_colmajor"]["ms_median"]
    results["e_host_loop_of_gg_get_layers"] = {"slots": n_get, "ms_wall": wall, "ms_for_all_maps": per_1024, "ratio_to_c_shipped_colmajor": per_1024 / c_ms}
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
