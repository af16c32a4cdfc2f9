#!/usr/bin/env python3
"""gg_import_layers on the headline shape (1024 maps of 364 x 364 after one default batch): the tiled kernel against the source-ordered
scatter (gg_debug_set_tuning "import_variant"), both plane orders, timed by stream events, next to three yardsticks:

  * gg_export_layers of the same mask on the same box (the same bytes in the other direction),
  * the scatter variant,
  * a host loop of gg_set_layer over the same maps and layers (what a caller had before; gg_set_layer is the code of the parent commit),
    by the wall clock.

Masks: (a) ground + groundpatch   (b) all eleven   (c) the nine per-call layers.  The default batch runs again in front of every timed
import (outside the timed interval), so that every import meets the sparse per-call layers and the pending lazily kept layers a batch
leaves -- an import makes the maps dense, the next one would otherwise find nothing left to fill.  The source planes are an export of the
maps themselves.

Bytes are what the call has to move, from the shapes: 4 per cell and plane read, 8 per cell for the interleaved pairs when ground or
groundpatch is named (4 when only one of them is), 4 per cell and per-call layer written (a lower bound: the dead half columns of the
layers that are not named are filled as well).  Needs a GPU; writes one JSON file and prints it.

    python tools/bench_import.py --out profiles/import_layers/import_layers.json
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
PERCALL = [k for k in LAYERS if k not in ("ground", "groundpatch")]
CASES = {"a_ground_groundpatch": ["ground", "groundpatch"], "b_all_eleven": list(LAYERS), "c_nine_percall": PERCALL}


def nominal_bytes(names, n_maps, cells):
    gp = 4 * sum(1 for k in names if k in ("ground", "groundpatch"))
    percall = sum(1 for k in names if k not in ("ground", "groundpatch"))
    return n_maps * cells * (gp + 4 * percall + 4 * len(names))


def stats(t, nb):
    t = np.array(t)
    med = float(np.median(t))
    return {"ms_median": med, "ms_min": float(t.min()), "ms_max": float(t.max()), "spread_ms": float(t.max() - t.min()),
            "TBs": nb / (med * 1e-3) / 1e12, "share_of_copy_ceiling": nb / (med * 1e-3) / 1e12 / COPY_CEILING_TBS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--setter-slots", type=int, default=64, help="slots of the gg_set_layer loop (0 = all); its time is scaled to all maps")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_import.py needs a GPU")
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
        src_all = torch.empty((B * len(LAYERS) * cells,), dtype=torch.float32, device="cuda")
        dst_all = torch.empty_like(src_all)
        for case, names in CASES.items():
            K = len(names)
            shape = {False: (B, K, seg.cols, seg.rows), True: (B, K, seg.rows, seg.cols)}
            src = {rm: src_all[: B * K * cells].view(shape[rm]) for rm in (False, True)}
            events = {}
            for row_major in (False, True):
                out = seg.filter_batch(pts, n_pts, origins, base_z, out=out)
                seg.export_layers(names, out=src[row_major], row_major=row_major)  # (the planes the imports of this order read)
                for rep in range(-args.warmup, args.reps):
                    for variant in (0, 1):  # (alternating: both see the same neighbours on the machine)
                        seg.debug_set_tuning("import_variant", variant)
                        out = seg.filter_batch(pts, n_pts, origins, base_z, out=out)  # (sparse layers, the three lazy ones pending)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        seg.import_layers(src[row_major], names, row_major=row_major)
                        e1.record()
                        if rep >= 0:
                            events.setdefault(("scatter" if variant else "tiled", row_major), []).append((e0, e1))
                    # the same bytes in the other direction, from the state a batch leaves as well
                    out = seg.filter_batch(pts, n_pts, origins, base_z, out=out)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    seg.export_layers(names, out=dst_all[: B * K * cells].view(shape[row_major]), row_major=row_major)
                    e1.record()
                    if rep >= 0:
                        events.setdefault(("export", row_major), []).append((e0, e1))
                stream.synchronize()  # (once per case and order: the device never idles between repetitions)
            seg.debug_set_tuning("import_variant", seg.debug_set_tuning("import_variant_default", 0))
            nb = nominal_bytes(names, B, cells)
            entry = {"layers": K, "bytes_nominal": nb, "runs": {}}
            for (what, row_major), ev in sorted(events.items()):
                entry["runs"][f"{what}_{'rowmajor' if row_major else 'colmajor'}"] = stats([a.elapsed_time(b) for a, b in ev], nb)
            results["cases"][case] = entry
    stream.synchronize()
    shipped = "scatter" if seg.debug_set_tuning("import_variant_default", 0) else "tiled"
    results["shipped_variant"] = shipped
    # what a caller had before: one gg_set_layer per slot and layer, from the host
    n_set = args.setter_slots or B
    planes = {name: np.asfortranarray(np.random.default_rng(5).random((seg.rows, seg.cols), dtype=np.float32)) for name in LAYERS}
    loop = {}
    for case, names in CASES.items():
        out = seg.filter_batch(pts, n_pts, origins, base_z, out=out)
        seg.synchronize()
        for name in names:
            seg.map(B - 1).set(name, planes[name])
        t0 = time.perf_counter()
        for s in range(n_set):
            for name in names:
                seg.map(s).set(name, planes[name])
        wall = (time.perf_counter() - t0) * 1e3
        per_all = wall * B / n_set
        loop[case] = {"slots": n_set, "ms_wall": wall, "ms_for_all_maps": per_all,
                      "ratio_to_shipped_colmajor": per_all / results["cases"][case]["runs"][f"{shipped}_colmajor"]["ms_median"]}
    results["host_loop_of_gg_set_layer"] = loop
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
