#!/usr/bin/env python
"""bench.py -- point clouds/s through the GroundGrid hot path on N x MI355X (one process per GPU).

A "step" = one pass of filter_cloud semantics (src/GroundSegmentation.cpp:50-197) over one batch of independent
(cloud, map-state) pairs per GPU: BASELINE.json configs[1] (synthetic Velodyne HDL-64E, ~120 k points, 120 m / 0.33 m grid
-> 364 x 364 cells), `--batch` clouds per GPU per step, every cloud meeting a FRESHLY INITIALISED map (the "cold" contract
case of SURVEY.md 8(d): ground := 0, groundpatch := 1e-7, GroundGrid.cpp:71-75; the re-initialisation of the persistent state
is part of the timed step).  The clouds ROTATE over the map slots from step to step (cloud b meets slot (b + 37 i) mod B in
step i, gg_batch.slots), so no map sees the same cloud twice in a row: the tiles K2 has to clean change every step, as they
do for a driving vehicle.  Inputs are resident in HBM (packed 16-B records) before the timed region.  For N > 1 the clouds
shard across ranks (no data-path collective) and each step ends with one RCCL all-gather of the 2-bit label masks
(BASELINE.json configs[2]).  Rank 0 prints ONE JSON line; besides the headline it carries

  roofline        dominant KERNEL of the timed steps: algorithmic GB/s vs the 8 TB/s HBM peak (+ PMC traffic from profiles/)
  kernels         every kernel: avg ms per launch, algorithmic bytes, fraction of peak;  scatter_read_frac (north star)

and, with --full only (a plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line):

  roofline.traffic   measured by two rocprofv3 --pmc child runs of the headline instead of read from profiles/
  parity_checked_in_run   the TIMED batch's own outputs (labels, returned-cloud order, counts, ground, groundpatch of sampled
                  slots after the last timed step) against the oracle, bit-exact
  warm_map        the steady state (clouds keep rotating over warm maps), sampled slots replayed on the oracle
  config3         BASELINE configs[2]: 64 clouds in total, sharded 64 / N per GPU, fresh maps, all-gather of the masks
  config4         BASELINE configs[3]: dense 2.1 M-point clouds on a 1000 x 1000 grid, a GPU-filling batch and one cloud
  host_api        the drop-in call gg_filter_cloud (host buffers in and out over PCIe): synchronous, pipelined, and the
                  reference-typed binding's shape (sync call + download of all 11 layers)
  cpu_baseline    the oracle (1 thread) on the same clouds on this box's host cores (cold and warm);  cpu_baseline_8p4: the
                  reference's default 8 + 4 thread shape (timing only)

  python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B]        (N > 1: re-launches itself under torch.distributed.run)
  python bench.py --full                              every leg above
  python bench.py --dump-outputs DIR                  + DIR/<name>.npy: what the last timed step computed (dump_outputs)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W
  python bench.py --kitti-dir <.../sequences/00>     BASELINE configs[0] / configs[4]: replay a SemanticKITTI sequence
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
ROT = 37               # slots a cloud advances per step (see the module docstring)
N_SCENES = 32          # distinct ray-cast scenes per GPU; the other clouds of a batch are yaw rotations of them
DUMP_CLOUDS = 16       # --dump-outputs: clouds of the last timed step whose outputs are written (a seeded sample of the batch)


def make_clouds(batch: int, rank: int, n_scenes: int = N_SCENES, seed0: int = 20240113):
    """`batch` distinct synthetic HDL-64E clouds: n_scenes ray-cast scenes (seeds 20240113 + ...) x yaw rotations."""
    from groundgrid_amd import synth

    scenes = [synth.hdl64_cloud(seed=seed0 + rank * n_scenes + k) for k in range(min(n_scenes, batch))]
    clouds = []
    for b in range(batch):
        base = scenes[b % len(scenes)]
        rot = b // len(scenes)
        if rot == 0:
            clouds.append(base)
            continue
        ang = np.float32(2.0 * np.pi * rot / max(1, (batch + len(scenes) - 1) // len(scenes)) + 0.01 * b)
        c, s = np.cos(ang), np.sin(ang)
        out = synth.clone_cloud(base)
        out["x"] = (c * base["x"] - s * base["y"]).astype(np.float32)
        out["y"] = (s * base["x"] + c * base["y"]).astype(np.float32)
        clouds.append(out)
    return clouds


def algorithmic_bytes(n_pts, n_in, n_kept, C, T, nch, full_layers=True, cold=True):
    """minimal compulsory traffic per cloud, per kernel (bytes).  The sort kernels have no row of their own
    in 8(d) (their bytes are part of K2's 20 N): scan = the chunk histograms read and written once, scatter = one (z, key)
    record read and written per in-map point.  cold: every map of the step is freshly initialised -- no confidence anywhere, so the
    line-of-sight test (:243-275) cannot fire and k_classify does not gather the old ground: the 4 N_in of 8(d)'s K1 row are not
    compulsory there and are not counted."""
    return {
        "k_classify": 16 * n_pts + (0 if cold else 4 * n_in) + 4 * n_pts + 1 * n_pts,
        "k_scan": 2 * 4 * nch * T,
        "k_scatter": 8 * n_in + 8 * n_in,
        "k_reduce": 8 * n_in + (9 if full_layers else 6) * 4 * C,
        "k_patch": 6 * 4 * C + 2 * 4 * C,  # reads points, variance, minGroundHeight, ground, groundpatch, expectedPoints; writes ground,
                                           # groundpatch (`variance`, :323, is written by k_reduce and counted there)
        "k_sweep": 2 * 2 * 4 * C,
        "k_label": 16 * n_pts + 4 * n_pts + 8 * n_pts + 1 * n_pts,
    }


def kernel_table(ktimes, alg, clouds_per_launch):
    """avg ms per launch, algorithmic bytes and fraction of the HBM peak per kernel.  When the front end ran as fewer launches
    (k_scan and / or k_scatter inside k_classify: their launch counts are 0) their algorithmic bytes move to k_classify."""
    alg = dict(alg)
    for k in ("k_scan", "k_scatter"):
        if k in ktimes and ktimes[k][1] == 0:
            alg["k_classify"] += alg[k]
            alg[k] = 0
    ktimes = {k: v for k, v in ktimes.items() if v[1] > 0}
    rows = {}
    for k, (ms, launches) in ktimes.items():
        avg = ms / max(1, launches)
        bytes_per_launch = alg[k] * clouds_per_launch
        gbs = bytes_per_launch / (avg * 1e-3) / 1e9 if avg > 0 else 0.0
        rows[k] = {"avg_ms": round(avg, 4), "alg_MB_per_launch": round(bytes_per_launch / 1e6, 2), "GBps": round(gbs, 1),
                   "frac_hbm": round(gbs / HBM_PEAK_GBS, 4)}
    return rows


LIVE_PMC = {}  # kernel -> corrected HBM bytes per cloud, measured by THIS run (live_pmc_passes); empty: the committed profile is used


def live_pmc_passes(batch, timeout_s=90):
    """The HBM traffic of every kernel of the headline workload, measured by this run on this box: two child runs of this script
    (headline only, 3 timed steps) under `rocprofv3 --pmc FETCH_SIZE --kernel-trace` and `--pmc WRITE_SIZE --kernel-trace` -- separate
    passes, counters with the kernel trace only, collected and corrected as /opt/skills/guides/MI355X_MICROARCH.md's HBM section
    prescribes (tools/pmc_summary.py: the cold first launch of a kernel dropped, FETCH doubled for the kernels whose wide coalesced
    streams gfx950 counts at half).  Returns {"source": ..., "kernels": {name: bytes per cloud}} or a dict with "error" (no rocprofv3,
    a pass failed or ran out of time: the committed profile is used instead, and the line says so)."""
    import importlib.util
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not exe:
        return {"error": "rocprofv3 not found"}
    spec = importlib.util.spec_from_file_location("gg_pmc_summary", os.path.join(ROOT, "tools", "pmc_summary.py"))
    pmc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pmc)
    out = {}
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        env = dict(os.environ, TMPDIR="/tmp")
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--",
                   sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-extras", "--no-live-pmc", "--batch", str(batch)]
            try:
                subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            except Exception as e:  # (a profiler that is missing a counter, a box without the PMC interface, a timeout)
                return {"error": f"{counter} pass: {type(e).__name__}"}
            found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("counter_collection.csv")]
            if not found:
                return {"error": f"{counter} pass wrote no counter_collection.csv"}
            out[counter] = pmc.per_kernel(found[0])
    kernels = {}
    for k in pmc.KERNELS:
        if k in out["FETCH_SIZE"] and k in out["WRITE_SIZE"]:
            f = out["FETCH_SIZE"][k] * 1024.0 * (2.0 if k in pmc.HALVED else 1.0)
            w = out["WRITE_SIZE"][k] * 1024.0
            kernels[k] = (f + w) / batch
    if not kernels:
        return {"error": "no kernel of the path in the counter files"}
    return {"source": "live: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; --kernel-trace only) of this script's headline workload, spawned by this run "
                      "on this box", "seconds": round(time.perf_counter() - t0, 1), "kernels": kernels}


def pmc_traffic(kernel, clouds_per_launch, section="kernels"):
    """HBM bytes per launch of `kernel`: measured by this run (live_pmc_passes) when it could, else from the committed rocprofv3 --pmc
    passes (profiles/pmc_summary.json; `section` "kernels" = the headline workload, "config4_kernels" = configs[3]), scaled to this
    launch size; None when neither knows the kernel."""
    if section == "kernels" and kernel in LIVE_PMC:
        return int(LIVE_PMC[kernel] * clouds_per_launch)
    path = os.path.join(ROOT, "profiles", "pmc_summary.json")
    try:
        summary = json.load(open(path))
        per_cloud = summary[section][kernel]["hbm_bytes_per_cloud"]
        return int(per_cloud * clouds_per_launch)
    except Exception:
        return None


def add_real_traffic(table, clouds_per_launch, section="kernels"):
    """Per kernel: the bytes it REALLY moved (PMC, profiles/pmc_summary.json) next to the algorithmic ones: `real_frac` = PMC
    bytes / time / peak, `traffic_ratio` = PMC / algorithmic bytes (> 1: re-reads or read-modify-writes; < 1: the kernel does
    not move what SURVEY 8(d) counts for it -- e.g. k_reduce never writes dead half columns).  Returns the whole step's real
    fraction of the HBM peak (None without a committed profile of every kernel)."""
    total, complete = 0.0, True
    for k, row in table.items():
        t = pmc_traffic(k, clouds_per_launch, section)
        if t is None or row["avg_ms"] <= 0:
            complete = False
            continue
        row["pmc_MB_per_launch"] = round(t / 1e6, 2)
        row["real_frac_hbm"] = round(t / (row["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        row["traffic_ratio"] = round(t / max(1.0, row["alg_MB_per_launch"] * 1e6), 3)
        total += t
    ms = sum(r["avg_ms"] for r in table.values())
    return round(total / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if complete and ms > 0 else None


def ordered_line(result, world):
    """The JSON line with what a reader needs FIRST and LAST: the contract's fields, then a compact `summary` (the legs whose
    numbers sit deep inside the long per-kernel tables: host API, single-cloud latency, configs[2] / [3], parity flags), then
    `roofline` and `cpu_baseline`, then the long tables, and the same summary again as the line's tail -- a log window cut to the
    first or the last two kilobytes still shows every headline number (`host_api` was cut out of both)."""
    def pick(d, *path):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return d

    summary = {
        "clouds_per_s": result.get("value"), "n1_equivalent": round(result["value"] / max(1, world), 2) if "value" in result else None,
        "ms_per_step": result.get("ms_per_step"),
        "warm_clouds_per_s": pick(result, "warm_map", "clouds_per_s"),
        "dominant_kernel": pick(result, "roofline", "kernel"), "roofline_frac": pick(result, "roofline", "frac"),
        "roofline_real_frac": pick(result, "roofline", "real_frac"), "step_real_frac_hbm": result.get("step_real_frac_hbm"),
        "all_kernels_frac_hbm": result.get("all_kernels_frac_hbm"),
        "scatter_read_frac": pick(result, "scatter_read_frac", "frac"), "front_end_frac": pick(result, "scatter_read_frac", "front_end_frac"),
        "insert_ms": pick(result, "scatter_read_frac", "insert_ms"),
        "kernel_ms": {k.replace("k_", ""): v["avg_ms"] for k, v in (result.get("kernels") or {}).items()},
        "cpu_1thread_clouds_per_s": {"cold": pick(result, "cpu_baseline", "value"), "warm": pick(result, "cpu_baseline_warm", "value")},
        "speedup_vs_cpu_1thread": {"cold": pick(result, "speedup_vs_cpu_1thread", "cold_over_cold"), "warm": pick(result, "speedup_vs_cpu_1thread", "warm_over_warm")},
        "host_api_clouds_per_s": {k: pick(result, "host_api", k + "_clouds_per_s") for k in ("sync", "pipelined", "binding_like", "binding_like_registered", "pc2_out", "device_resident_binding")},
        "host_api_vs_cpu_1thread": {"sync": pick(result, "host_api", "sync_vs_cpu_1thread"), "pipelined": pick(result, "host_api", "vs_cpu_1thread"),
                                    "binding_like": pick(result, "host_api", "binding_like_vs_cpu_1thread"),
                                    "device_resident_binding": pick(result, "host_api", "device_resident_binding_vs_cpu_1thread")},
        "single_cloud_latency_ms": result.get("single_cloud_latency_ms"),
        "concurrent_halves_clouds_per_s": pick(result, "concurrent_halves", "clouds_per_s"),
        "eager_layers": {"clouds_per_s": pick(result, "eager_layers", "clouds_per_s"), "reduce_ms": pick(result, "eager_layers", "kernel_ms", "k_reduce")},
        "lazy_read_materialise_ms_per_map": pick(result, "lazy_layers", "materialise_ms_per_map"),
        "warm_map_unrelated_scenes": {"clouds_per_s": pick(result, "warm_map_unrelated_scenes", "clouds_per_s"), "k_classify_ms": pick(result, "warm_map_unrelated_scenes", "kernel_ms", "k_classify")},
        "roofline_traffic_source": pick(result, "roofline", "traffic_source"),
        "config3_clouds_per_s": pick(result, "config3", "clouds_per_s"),
        "config4": {"clouds_per_s": pick(result, "config4", "clouds_per_s"), "all_kernels_frac_hbm": pick(result, "config4", "all_kernels_frac_hbm"),
                    "dominant_frac": pick(result, "config4", "roofline", "frac"), "single_cloud_latency_ms": pick(result, "config4", "single_cloud", "latency_ms"),
                    "cpu_clouds_per_s": pick(result, "config4", "cpu_baseline", "value")},
        "config5_synthetic": {"frames": pick(result, "config5_synthetic", "frames"), "clouds_per_s": pick(result, "config5_synthetic", "clouds_per_s"),
                              "cpu_clouds_per_s": pick(result, "config5_synthetic", "cpu_baseline", "value"),
                              "final_map_identical": pick(result, "config5_synthetic", "final_map_identical")},
        "parity_checked_in_run": {"headline": result.get("parity_checked_in_run"), "config5_synthetic": pick(result, "config5_synthetic", "parity_checked_in_run"), "warm": pick(result, "warm_map", "parity_checked_in_run"),
                                  "config3": pick(result, "config3", "parity_checked_in_run"), "config4": pick(result, "config4", "parity_checked_in_run"),
                                  "lazy_layers": pick(result, "lazy_layers", "parity_checked_in_run"), "eager_layers": pick(result, "eager_layers", "parity_checked_in_run"), "concurrent_halves": pick(result, "concurrent_halves", "parity_checked_in_run"),
                                  "config4_single": pick(result, "config4", "single_cloud", "parity_checked_in_run")},
    }
    head = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"]
    out = {k: result[k] for k in head if k in result}
    out["summary"] = summary
    for k in ("roofline", "cpu_baseline"):
        if k in result:
            out[k] = result[k]
    for k, v in result.items():
        if k not in out:
            out[k] = v
    out["summary_tail"] = summary
    return out


def dump_outputs(directory, pipe, n_points):
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy.  counts [B, 4] of every cloud (float64);
    for DUMP_CLOUDS clouds drawn with a fixed seed (cloud_ids, and map_slots: the slots they met) their labels and out_index
    ([k, longest of them], -1 past a cloud's end) and the ground and groundpatch layers of their maps ([k, rows, cols]), float32 --
    exact, as labels and indices are integers below 2^24 and the layers are float32 themselves.  About 34 MB for the headline."""
    os.makedirs(directory, exist_ok=True)
    out, last = pipe.out, pipe.shifts[-1]
    ids = np.sort(np.random.default_rng(0).choice(pipe.nb, size=min(DUMP_CLOUDS, pipe.nb), replace=False))
    slots = [pipe.slot_of(int(b), last) for b in ids]
    width = max(1, max(int(n_points[b]) for b in ids))
    labels = np.full((len(ids), width), -1.0, dtype=np.float32)
    index = np.full((len(ids), width), -1.0, dtype=np.float32)
    for i, b in enumerate(ids):
        n = int(n_points[b])
        labels[i, :n] = out.labels[b, :n].cpu().numpy()
        index[i, :n] = out.out_index[b, :n].cpu().numpy()
    arrays = {
        "counts": out.counts.cpu().numpy().astype(np.float64),
        "cloud_ids": ids.astype(np.float64),
        "map_slots": np.asarray(slots, dtype=np.float64),
        "labels": labels,
        "out_index": index,
        "ground": np.stack([pipe.seg.map(s)["ground"] for s in slots]).astype(np.float32),
        "groundpatch": np.stack([pipe.seg.map(s)["groundpatch"] for s in slots]).astype(np.float32),
    }
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def relaunch_under_torchrun(n: int):
    """`python bench.py --gpus N` without a launcher: become `python -m torch.distributed.run --nproc-per-node N bench.py ...`
    (one process per GPU), the command line the driver uses for N > 1."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.execvp(cmd[0], cmd)


def nan_equal(a, b):
    return bool(np.array_equal(a, b, equal_nan=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="independent (cloud, map) pairs per GPU per step")
    ap.add_argument("--full", action="store_true", help="every leg: the live PMC passes, the oracle checks of the timed outputs, warm / "
                    "halves / layers / config3 / config4 / host_api / CPU legs and the synthetic drive (a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps write what the last one computed as "
                    "DIR/<name>.npy (float32 / float64): counts of every cloud; labels, out_index, ground and groundpatch of a seeded sample")
    ap.add_argument("--eager-layers", action="store_true", help="GG_FLAG_EAGER_LAYERS: maintain all nine per-call layers for every cloud (the library's default for "
                    "gg_filter_batch leaves the three that nothing on the path reads to their first reader)")
    ap.add_argument("--minimal-layers", action="store_true", help="(the default since round 6; kept for old command lines)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="CPU baseline budget (rank 0, N=1 only)")
    ap.add_argument("--no-profile", action="store_true", help="do not bracket kernels with HIP events")
    ap.add_argument("--no-extras", action="store_true", help="headline only (no warm / config3 / config4 / host_api / CPU legs)")
    ap.add_argument("--no-live-pmc", action="store_true", help="do not spawn the two rocprofv3 --pmc passes that measure roofline.traffic on this box "
                                                               "(the committed profile's figures are used)")
    ap.add_argument("--no-rotate", action="store_true", help="every step applies cloud b to slot b (round 2's workload)")
    ap.add_argument("--config4-batch", type=int, default=128, help="clouds per launch of the configs[3] leg (GPU-filling)")
    ap.add_argument("--abi-collective", action="store_true", help="all-gather through the C ABI (gg_allgather_label_masks, RCCL bound by the "
                    "library itself) instead of torch.distributed")
    ap.add_argument("--gather", choices=["all", "config3-only"], default="all",
                    help="N > 1: 'all' = every headline step ends with the all-gather of its label masks (overlapped with the next step); "
                         "'config3-only' = the headline steps run without a collective (kernel scaling alone), only the configs[2] leg gathers")
    ap.add_argument("--force-dist", action="store_true", help="run the N > 1 code path (RCCL process group, all-gather per step) even with one rank")
    ap.add_argument("--dry-launch", action="store_true", help="rendezvous of the N ranks only (gloo when no GPU is visible): launch-path check")
    ap.add_argument("--only-config4", action="store_true", help="profiling runs: a token headline (8 clouds), then only the configs[3] leg")
    ap.add_argument("--drive-frames", type=int, default=4540, help="frames of the configs[4]-shaped synthetic drive leg (0: skip it)")
    ap.add_argument("--kitti-dir", default=None, help="SemanticKITTI sequence directory: replay it instead of the synthetic bench")
    ap.add_argument("--kitti-max-frames", type=int, default=0)
    ap.add_argument("--kitti-euler-roundtrip", action="store_true", help="model the player's quaternion -> euler -> quaternion round trip")
    args = ap.parse_args()
    if args.only_config4:
        args.batch, args.steps, args.warmup = 8, 2, 1

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        relaunch_under_torchrun(args.gpus)  # does not return

    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)

    if args.dry_launch:
        import torch.distributed as dist_mod

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        on_gpu = torch.cuda.is_available() and torch.cuda.device_count() >= world
        if on_gpu:
            torch.cuda.set_device(local_rank)
        if world > 1 or "MASTER_PORT" in os.environ:
            dist_mod.init_process_group(backend="nccl" if on_gpu else "gloo", rank=rank, world_size=world)
            t = torch.tensor([rank + 1], dtype=torch.int64, device=f"cuda:{local_rank}" if on_gpu else "cpu")
            dist_mod.all_reduce(t)
            ok = int(t.item()) == world * (world + 1) // 2
            backend = dist_mod.get_backend()
            ranks = dist_mod.get_world_size()
            dist_mod.barrier()
            dist_mod.destroy_process_group()
        else:
            ok, backend, ranks = True, "none", 1
        if rank == 0:
            print(json.dumps({"dry_launch": True, "ranks": ranks, "backend": backend, "all_reduce_ok": ok}))
        sys.exit(0 if ok else 1)

    if not torch.cuda.is_available():
        print("bench.py: no GPU visible (the HIP path has no CPU fallback)", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if args.kitti_dir:
        return kitti_leg(args, local_rank)

    dist = None
    if world > 1 or args.force_dist:  # (--force-dist: the multi-GPU code path -- RCCL process group, async gathers -- with ONE rank)
        import torch.distributed as dist_mod

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        dist = dist_mod
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)

    from groundgrid_amd import api
    from groundgrid_amd.dist import AbiLabelGather, common_stride, shard_range, unpack_label_masks

    class StreamGather:
        """gg_allgather_label_masks on a side stream (the library orders it after the batch that wrote the masks); wait() makes
        the compute stream wait for it -- the same contract as the torch.distributed work handle it replaces."""

        def __init__(self, gatherer):
            self.g, self.stream = gatherer, torch.cuda.Stream(device=dev)

        def __call__(self, out, masks):
            self.g.gather(masks, out=out, stream=self.stream.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(self.stream)

            class Handle:
                def wait(self_inner):
                    torch.cuda.current_stream(dev).wait_event(ev)

            return Handle()

    B = args.batch
    clouds = make_clouds(B, rank)
    n_points = [len(c) for c in clouds]
    stride = common_stride(max(n_points), device=dev)  # one shape on every rank; multiple of 64 (2-bit masks need 4)
    seg = api.GroundSegmentation().init(120.0, 0.33, n_slots=B, max_points=stride, device=local_rank)
    seg.set_flags(eager_layers=args.eager_layers, profile=not args.no_profile)

    def to_device(cl, st):
        host = np.zeros((max(len(cl), 1), st), dtype=api.POINT16_DTYPE)
        for b, c in enumerate(cl):
            host[b, : len(c)] = api.pack16(c)
        return torch.from_numpy(host.view(np.uint8).reshape(host.shape[0], st, 16)).to(dev)[: len(cl)].contiguous()

    points = to_device(clouds, stride)
    origins = np.zeros((B, 3), dtype=np.float32)
    base_z = np.full(B, -1.73)

    class Pipeline:
        """Double-buffered outputs: the all-gather of step i's label masks (RCCL's own stream, async_op) overlaps step i+1's
        kernels; buffer i % 2 is reused only after its gather completed.  shifts[i] = how far the clouds were rotated over the
        slots in step i (cloud b -> slot (b + shift) mod nb)."""

        def __init__(self, seg_, pts, npts, org, bz, cold, rotate=True, first_shift=0, within_halves=False, gather=True):
            self.seg, self.pts, self.npts, self.org, self.bz, self.cold = seg_, pts, npts, org, bz, cold
            self.gather = gather and dist is not None  # (--gather config3-only: the headline's steps end without the collective)
            self.within_halves = within_halves  # the clouds rotate over the slots of their own half (a row of the outputs keeps its half)
            self.outs, self.pending, self.step_no, self.out = [None, None], [None, None], 0, None
            self.nb = nb = pts.shape[0]
            self.rotate = rotate and not args.no_rotate and nb > 1
            self.shift = first_shift
            self.shifts = []
            self.ids = np.arange(nb, dtype=np.int64)
            self.gathered = [torch.empty((world * nb, pts.shape[1] // 4), dtype=torch.uint8, device=dev) for _ in range(2)] if self.gather else None
            self.abi = StreamGather(AbiLabelGather(seg_, rank, world)) if (self.gather and args.abi_collective) else None

        def slots_of(self, shift):
            if self.within_halves:
                h = self.nb // 2
                return np.where(self.ids < h, (self.ids + shift) % h, h + (self.ids - h + shift) % (self.nb - h)).astype(np.int32)
            return ((self.ids + shift) % self.nb).astype(np.int32)

        def slot_of(self, b, shift):
            return int(self.slots_of(shift)[b])

        def step(self):
            k = self.step_no % 2
            if self.pending[k] is not None:
                self.pending[k].wait()  # orders the compute stream after the gather that still reads outs[k].label_masks
                self.pending[k] = None
            if self.cold:  # every cloud meets a freshly initialised map: ground := 0, groundpatch := 1e-7 (one launch, timed)
                self.seg.reset_maps(0, self.nb, odom_z=0.0, persistent_only=True, on_torch_stream=True)
            if self.rotate:
                self.shift = (self.shift + ROT) % self.nb
            self.shifts.append(self.shift)
            self.outs[k] = self.seg.filter_batch(self.pts, self.npts, self.org, self.bz, out=self.outs[k], want_masks=self.gather,
                                                 slots=self.slots_of(self.shift) if (self.rotate or self.shift) else None)
            self.out = self.outs[k]
            if self.abi:
                self.pending[k] = self.abi(self.gathered[k], self.outs[k].label_masks)
            elif self.gather:
                self.pending[k] = dist.all_gather_into_tensor(self.gathered[k], self.outs[k].label_masks, async_op=True)
            self.step_no += 1

        def fence(self):
            for k in range(2):
                if self.pending[k] is not None:
                    self.pending[k].wait()
                    self.pending[k] = None
            self.seg.synchronize()
            torch.cuda.synchronize(dev)
            if dist:
                dist.barrier()
                torch.cuda.synchronize(dev)

        def timed(self, steps, warmup):
            for _ in range(warmup):
                self.step()
            self.fence()
            if not args.no_profile:
                self.seg.kernel_times(reset=True)
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step()
            self.fence()
            elapsed = time.perf_counter() - t0
            if dist:
                t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                elapsed = float(t.item())
            kt = self.seg.kernel_times(reset=True) if not args.no_profile else {}
            return elapsed, kt

    def check_timed_outputs(pipe, cl, length, resolution, history_of=None, n_check=8, seed=1):
        """The outputs the timed steps left behind against the oracle, bit-exact: labels, returned-cloud order and counts of
        `n_check` random clouds of the LAST step's batch, and the ground / groundpatch / variance / points layers of the maps
        they met.  history_of(slot) -> the clouds (indices) that slot saw since its last reset, in order (default: the last
        step's cloud on a fresh map = a cold step)."""
        from oracle import oracle

        rng = np.random.default_rng(seed)
        nb = pipe.nb
        last = pipe.shifts[-1]
        labels, index, counts = pipe.out.labels, pipe.out.out_index, pipe.out.counts.cpu().numpy()
        ok, checked = True, []
        for b in sorted(rng.choice(nb, size=min(n_check, nb), replace=False).tolist()):
            slot = pipe.slot_of(b, last)
            hist = history_of(slot) if history_of else [b]
            ref = oracle.OracleMap(length, resolution)
            r = None
            for cb in hist:
                r = ref.filter_cloud(cl[cb], (0.0, 0.0, 0.0), -1.73)
            assert hist[-1] == b
            n = len(cl[b])
            good = bool(np.array_equal(labels[b, :n].cpu().numpy(), r["label"]) and np.array_equal(index[b, :n].cpu().numpy(), r["index"]))
            good &= int(counts[b, 0]) == len(r["out_points"]) and int(counts[b, 3]) == int((r["cls"] == oracle.OUTLIER).sum())
            m = pipe.seg.map(slot)
            for layer in ("ground", "groundpatch", "variance", "points"):
                good &= nan_equal(m[layer], ref.layer(layer))
            ok &= good
            checked.append({"cloud": b, "slot": slot, "frames": len(hist), "ok": good})
        return ok, checked

    # ---------------------------------------------------------------- headline: cold maps, K timed steps
    gather_headline = args.gather == "all"
    pipe = Pipeline(seg, points, n_points, origins, base_z, cold=True, gather=gather_headline)
    elapsed, ktimes = pipe.timed(args.steps, args.warmup)
    total_clouds = world * B * args.steps
    value = total_clouds / elapsed

    result = {
        "metric": "point clouds/s (Velodyne-64, ~120k pts, 120m/0.33m grid)",
        "value": round(value, 2),
        "unit": "clouds/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32+f64 (the reference's mixed float/double arithmetic, bit-exact)",
        "data": f"synthetic (seeded HDL-64E ray caster, {min(N_SCENES, B)} scenes x yaw rotations per GPU; no dataset on the box)",
        "config": {
            "workload": "BASELINE configs[1]: synthetic Velodyne HDL-64E cloud, 364x364 grid @ 0.33 m, "
                        f"{B} independent (cloud, map-state) pairs per GPU per step, COLD maps (each step re-initialises the persistent "
                        "state of its maps -- ground 0, groundpatch 1e-7 -- inside the timed region, then filters)"
                        + ("" if args.no_rotate else f"; the clouds rotate over the map slots by {ROT} per step")
                        + ("; + RCCL all-gather of the 2-bit label masks per step (configs[2])" if (world > 1 and gather_headline) else "")
                        + ("; NO collective in these steps (--gather config3-only: the configs[2] leg carries it)" if (world > 1 and not gather_headline) else ""),
            "clouds_per_gpu_per_step": B,
            "points_per_cloud_mean": int(np.mean(n_points)),
            "grid": "364x364",
            "map_state": "cold",
            "point_format": "packed 16 B (x,y,z,ring) resident in HBM",
            "layers": "all 11 maintained for every cloud (GG_FLAG_EAGER_LAYERS)" if args.eager_layers else
                      "gg_filter_batch's default: the eight layers the path reads or rewrites maintained per cloud; groundCandidates, planeDist, maxGroundHeight "
                      "(read by nothing on the path) computed on their first read -- every getter returns the reference's values at all times",
            "parallelism": f"clouds sharded {B}/GPU x {world} GPU, no data-path collective"
                           + (", 1 all-gather of label masks per step overlapped with the next step" if (world > 1 and gather_headline) else ""),
        },
    }
    if dist:
        result["collective"] = {"backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(),
                                "issued_by": "gg_allgather_label_masks (C ABI, RCCL bound by the library)" if args.abi_collective else "torch.distributed",
                                "bytes_per_rank_per_step": int(B * stride // 4), "bytes_received_per_rank_per_step": int((world - 1) * B * stride // 4),
                                "in_headline_steps": bool(gather_headline)}

    rows, C = seg.rows, seg.rows * seg.rows
    T = ((rows + 15) // 16) ** 2
    if rank == 0 and ktimes:
        torch.cuda.synchronize(dev)
        counts = pipe.out.counts.cpu().numpy()
        n_mean = float(np.mean(n_points))
        n_in = float(np.mean(counts[:, 1] + counts[:, 2] + counts[:, 3]))  # emitted kept + ignored + outliers ~ in-map
        n_kept = float(np.mean(counts[:, 1]))
        pw = seg.debug_set_tuning("pw", 0)  # points per wave chunk of this context (K1 / scan / scatter / K5)
        alg = algorithmic_bytes(n_mean, n_in, n_kept, C, T, (stride + pw - 1) // pw, full_layers=args.eager_layers)
        table = kernel_table(ktimes, alg, B)
        traffic_source = "profiles/pmc_summary.json (the committed profile round, rescaled to this batch)"
        if world == 1 and dist is None and args.full and not args.no_extras and not args.no_live_pmc and not args.only_config4:
            live = live_pmc_passes(B)
            if "kernels" in live:
                LIVE_PMC.update(live["kernels"])
                traffic_source = live["source"] + f" ({live['seconds']} s)"
            else:
                traffic_source += f"; the live passes failed: {live['error']}"
        step_real = add_real_traffic(table, B)
        dominant = max(table, key=lambda k: table[k]["avg_ms"])
        g = table[dominant]
        result["roofline"] = {
            "kernel": dominant, "bound": "hbm", "achieved": g["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": g["frac_hbm"],
            "traffic": pmc_traffic(dominant, B), "real_frac": g.get("real_frac_hbm"), "traffic_ratio": g.get("traffic_ratio"),
            "traffic_source": traffic_source,
            "note": "dominant single kernel of the timed (cold) steps; achieved = SURVEY 8(d) algorithmic bytes x clouds per launch / its "
                    "average launch duration (HIP events on the launch stream inside the timed region); real_frac = the bytes the kernel "
                    "really moved (traffic: corrected PMC counters, see traffic_source) over the same duration, traffic_ratio = "
                    "traffic / algorithmic bytes",
        }
        front = [k for k in ("k_classify", "k_scan", "k_scatter") if k in table]
        insert_ms = sum(table[k]["avg_ms"] for k in front + ["k_reduce"])
        front_ms = sum(table[k]["avg_ms"] for k in front)
        read_gbs = 20.0 * n_mean * B / (insert_ms * 1e-3) / 1e9
        result["scatter_read_frac"] = {
            "frac": round(read_gbs / HBM_PEAK_GBS, 4), "GBps": round(read_gbs, 1), "insert_ms": round(insert_ms, 4),
            "front_end_launches": front, "front_end_ms": round(front_ms, 4),
            "front_end_frac": round(20.0 * n_mean * B / (front_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "note": "north star: SURVEY 8(d) scatter read figure 20 N bytes per cloud over the whole insert (front end + reduce); "
                    "front_end_frac = the same bytes over the scatter proper (classify + stable tile sort, front_end_launches)",
        }
        whole = sum(alg.values()) * B / (1e-3 * sum(r["avg_ms"] for r in table.values())) / 1e9
        result["all_kernels_frac_hbm"] = round(whole / HBM_PEAK_GBS, 4)
        result["step_real_frac_hbm"] = step_real
        result["kernels"] = table

    if rank == 0 and args.dump_outputs:  # (before any leg below touches the maps or the output buffers)
        dump_outputs(args.dump_outputs, pipe, n_points)

    extras = args.full and not args.no_extras and not args.only_config4
    do_checks = rank == 0 and extras and args.cpu_seconds > 0
    # ---------------------------------------------------------------- the timed batch's own outputs against the oracle
    if do_checks:
        ok, checked = check_timed_outputs(pipe, clouds, 120.0, 0.33)
        result["parity_checked_in_run"] = ok
        result["parity_check"] = {"what": "outputs of the LAST TIMED STEP of the headline batch vs the oracle, bit-exact: labels, returned-cloud "
                                          "order, counts, and the ground / groundpatch / variance / points layers of the slots the sampled clouds met",
                                  "sampled": checked}

    # ---------------------------------------------------------------- warm steady state, all ranks
    if extras:
        # The steady state of a drive: every map keeps meeting clouds of ITS scene (consecutive clouds of a vehicle overlap almost
        # entirely), so the clouds stay on the slots the last cold step left them on.  Rotating unrelated scenes over warm maps is
        # reported below as a stress case: the terrain of the previous scene then lies above a fifth of the new returns and every
        # one of them walks its line of sight (:246-275).
        cold_last = pipe.shifts[-1]
        warm = Pipeline(seg, points, n_points, origins, base_z, cold=False, rotate=False, first_shift=cold_last)
        w_steps = max(4, args.steps // 2)
        w_elapsed, w_kt = warm.timed(w_steps, 2)
        if rank == 0:
            result["warm_map"] = {"clouds_per_s": round(world * B * w_steps / w_elapsed, 1), "ms_per_step": round(1e3 * w_elapsed / w_steps, 4),
                                  "kernel_ms": {k: round(v[0] / max(1, v[1]), 4) for k, v in w_kt.items()},
                                  "note": "no re-initialisation: every map keeps its terrain and meets the same scene again in every step (the "
                                          "steady state of a drive)"}
            if do_checks:
                hist_shifts = [cold_last] + warm.shifts  # what every slot saw since its last reset (the cold leg's last step)
                okw, chk = check_timed_outputs(warm, clouds, 120.0, 0.33, n_check=2, seed=2,
                                               history_of=lambda slot: [int((slot - s) % B) for s in hist_shifts])
                result["warm_map"]["parity_checked_in_run"] = okw
                result["warm_map"]["parity_frames_replayed"] = len(hist_shifts)
        if not args.no_rotate and B > 1:
            mixed = Pipeline(seg, points, n_points, origins, base_z, cold=False, first_shift=cold_last)
            m_elapsed, m_kt = mixed.timed(3, 1)
            if rank == 0:
                result["warm_map_unrelated_scenes"] = {
                    "clouds_per_s": round(world * B * 3 / m_elapsed, 1), "ms_per_step": round(1e3 * m_elapsed / 3, 4),
                    "kernel_ms": {k: round(v[0] / max(1, v[1]), 4) for k, v in m_kt.items()},
                    "note": "stress: warm maps, but the clouds rotate over the slots, so every map meets a DIFFERENT scene in every step -- "
                            "k_classify then walks lines of sight for ~20 % of the returns"}
                if do_checks:
                    hs = [cold_last] + warm.shifts + mixed.shifts
                    result["warm_map_unrelated_scenes"]["parity_checked_in_run"] = check_timed_outputs(
                        mixed, clouds, 120.0, 0.33, n_check=1, seed=6, history_of=lambda slot: [int((slot - s) % B) for s in hs])[0]

    # ---------------------------------------------------------------- the headline's cold steps as two concurrent halves (a separate leg)
    if extras and rank == 0 and world == 1 and dist is None and B >= 512:
        # GG_FLAG_CONCURRENT_HALVES (include/groundgrid_hip.h): every call runs the clouds of the lower and of the upper half of the map
        # slots as two launch sequences on two streams that never join between steps, so kernels of different kinds overlap.  Reported
        # BESIDE the headline, not as it: with two kernels sharing the device a per-kernel event pair times half a machine, so this leg
        # has no per-kernel table and no roofline.
        seg.set_flags(eager_layers=args.eager_layers, profile=False, concurrent_halves=True)
        saved_no_profile, args.no_profile = args.no_profile, True
        h_steps = max(4, args.steps // 2)
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):  # (a real stream: the flag is ignored on the legacy default one)
            # halves / one sequence / halves / one sequence on the same stream, back to back, the same warm-up for each: the like-for-like
            # pairs; the faster run of either kind is reported.  The clouds rotate over the slots of their own half: a row of the output
            # buffers keeps its half, so the library need not join the two streams between steps (a row that changed its half would be
            # written from both: enqueue_batch orders such batches itself, and the overlap is gone)
            h_elapsed = one_seq = None
            shift = pipe.shifts[-1]
            for rep in range(2):
                seg.set_flags(eager_layers=args.eager_layers, profile=False, concurrent_halves=True)
                halves = Pipeline(seg, points, n_points, origins, base_z, cold=True, first_shift=shift, within_halves=True)
                e, _ = halves.timed(h_steps, 3)
                h_elapsed = e if h_elapsed is None else min(h_elapsed, e)
                seg.set_flags(eager_layers=args.eager_layers, profile=False)
                plain = Pipeline(seg, points, n_points, origins, base_z, cold=True, first_shift=halves.shifts[-1], within_halves=True)
                e, _ = plain.timed(h_steps, 3)
                one_seq = e if one_seq is None else min(one_seq, e)
                shift = plain.shifts[-1]
            seg.set_flags(eager_layers=args.eager_layers, profile=False, concurrent_halves=True)
            halves = Pipeline(seg, points, n_points, origins, base_z, cold=True, first_shift=shift, within_halves=True)
            halves.timed(2, 1)  # (the outputs check_timed_outputs reads: a divided run's)
        args.no_profile = saved_no_profile
        seg.set_flags(eager_layers=args.eager_layers, profile=not args.no_profile)
        result["concurrent_halves"] = {
            "clouds_per_s": round(world * B * h_steps / h_elapsed, 1), "ms_per_step": round(1e3 * h_elapsed / h_steps, 4),
            "one_sequence_same_stream_ms_per_step": round(1e3 * one_seq / h_steps, 4), "one_sequence_same_stream_clouds_per_s": round(world * B * h_steps / one_seq, 1),
            "note": "the headline's cold steps under gg_set_flags(GG_FLAG_CONCURRENT_HALVES): the clouds whose maps are in the lower / upper half "
                    "of the slots as two launch sequences on two streams, no join between steps (the caller fences before it reads outputs; the "
                    "clouds rotate over the slots of their own half, so that a row of the outputs keeps its half); each variant twice, "
                    "interleaved, same warm-up, the faster run of either; results identical; per-kernel timing is not meaningful in this mode"}
        if do_checks:
            result["concurrent_halves"]["parity_checked_in_run"] = check_timed_outputs(halves, clouds, 120.0, 0.33, n_check=4, seed=9)[0]

    # ---------------------------------------------------------------- all nine per-call layers for every cloud (a separate leg), and what a lazy read costs
    if extras and rank == 0 and world == 1 and not args.eager_layers:
        # SURVEY Appendix E / VERDICT r3 2(c), r5 5(a): by default k_reduce maintains the six per-call layers the path reads; maxGroundHeight,
        # groundCandidates and planeDist are computed when a reader asks (gg_get_layer), from the records the call left behind.
        lazy = Pipeline(seg, points, n_points, origins, base_z, cold=True)
        lazy.timed(2, 1)
        leg = {"note": "the library's default for gg_filter_batch; `materialise_ms_per_map`: the first read of one of the three published-only layers of a map "
                       "against a read of a maintained layer"}
        n_read = min(16, B)  # (a read = extract + 0.5 MB over PCIe; the lazy read also runs the three recurrences of that map first)
        t0 = time.perf_counter()
        for sl in range(n_read):
            seg.map(sl)["m2"]
        t1 = time.perf_counter()
        for sl in range(n_read):
            seg.map(sl)["planeDist"]
        t2 = time.perf_counter()
        leg["layer_read_ms"] = round(1e3 * (t1 - t0) / n_read, 4)
        leg["materialise_ms_per_map"] = round(1e3 * ((t2 - t1) - (t1 - t0)) / n_read, 4)
        if do_checks:
            from oracle import oracle
            okl, chk = check_timed_outputs(lazy, clouds, 120.0, 0.33, n_check=2, seed=4)
            for c in chk:  # ... and all 11 layers of those maps, the lazily computed ones among them
                ref = oracle.OracleMap(120.0, 0.33)
                ref.filter_cloud(clouds[c["cloud"]], (0.0, 0.0, 0.0), -1.73)
                got = seg.map(c["slot"]).layers()
                okl &= all(nan_equal(got[name], ref.layer(name)) for name in oracle.LAYERS)
            leg["parity_checked_in_run"] = bool(okl)
        result["lazy_layers"] = leg
        seg.set_flags(eager_layers=True, profile=not args.no_profile)
        eager = Pipeline(seg, points, n_points, origins, base_z, cold=True)
        l_steps = max(4, args.steps // 2)
        l_elapsed, l_kt = eager.timed(l_steps, 2)
        result["eager_layers"] = {"clouds_per_s": round(B * l_steps / l_elapsed, 1), "ms_per_step": round(1e3 * l_elapsed / l_steps, 4),
                                  "kernel_ms": {k: round(v[0] / max(1, v[1]), 4) for k, v in l_kt.items()},
                                  "note": "GG_FLAG_EAGER_LAYERS: all nine per-call layers written for every cloud (the headline of rounds 1-5)"}
        if do_checks:
            result["eager_layers"]["parity_checked_in_run"] = check_timed_outputs(eager, clouds, 120.0, 0.33, n_check=2, seed=14)[0]
        seg.set_flags(eager_layers=False, profile=not args.no_profile)

    # ---------------------------------------------------------------- configs[2]: 64 clouds in total, 64 / N per GPU
    if extras:
        first, cnt = shard_range(64, rank, world)
        c3_clouds = make_clouds(64, 0, n_scenes=8, seed0=20240113)[first:first + cnt]  # the same 64 clouds at every N
        c3_np = [len(c) for c in c3_clouds]
        c3_stride = common_stride(max(c3_np) if c3_np else 64, device=dev)
        seg3 = api.GroundSegmentation().init(120.0, 0.33, n_slots=max(cnt, 1), max_points=c3_stride, device=local_rank)
        p3 = to_device(c3_clouds, c3_stride) if cnt else None
        pipe3 = Pipeline(seg3, p3, c3_np, np.zeros((cnt, 3), np.float32), np.full(cnt, -1.73), cold=True, rotate=False)
        c3_steps = max(10, args.steps)
        e3, _ = pipe3.timed(c3_steps, 3)
        ok3 = None
        if dist:  # every rank now holds all 64 masks: hold the gathered copy of this rank's clouds to its own labels
            g = unpack_label_masks(pipe3.gathered[(pipe3.step_no - 1) % 2][first:first + cnt], c3_stride)
            ok3 = all(bool(torch.equal(g[b, : c3_np[b]], pipe3.out.labels[b, : c3_np[b]])) for b in range(cnt))
            t = torch.tensor([1 if ok3 else 0], device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            ok3 = bool(t.item())
        if rank == 0:
            result["config3"] = {"clouds_total": 64, "clouds_per_gpu": cnt, "clouds_per_s": round(64 * c3_steps / e3, 1),
                                 "ms_per_step": round(1e3 * e3 / c3_steps, 4), "scaling": "strong", "map_state": "cold",
                                 "gathered_masks_match_labels": ok3, "rccl_ranks": dist.get_world_size() if dist else 1,
                                 "note": "BASELINE configs[2]: 64 independent clouds sharded 64/N per GPU + one all-gather of the 2-bit "
                                         "label masks per step (N = 1: no collective)"}
            if do_checks:
                result["config3"]["parity_checked_in_run"] = check_timed_outputs(pipe3, c3_clouds, 120.0, 0.33, n_check=8, seed=3)[0]
        seg3.close()

    # ---------------------------------------------------------------- rank 0, N = 1: CPU legs, host API, config 4, latency
    if rank == 0 and world == 1 and extras and args.cpu_seconds > 0:
        from oracle import oracle

        n_cpu = min(B, 8)
        maps = [oracle.OracleMap(120.0, 0.33) for _ in range(n_cpu)]
        done, t_cpu0 = 0, time.perf_counter()
        while time.perf_counter() - t_cpu0 < args.cpu_seconds:
            for b in range(n_cpu):
                maps[b].reset_state()
                maps[b].filter_cloud(clouds[b], (0.0, 0.0, 0.0), -1.73)
            done += n_cpu
        t_cpu = time.perf_counter() - t_cpu0
        result["cpu_baseline"] = {
            "value": round(done / t_cpu, 2), "unit": "clouds/s", "cores": 1, "kind": "port",
            "sample": f"{done} filter_cloud calls over {n_cpu} of the batch's clouds, each on a freshly initialised map (cold, as the GPU "
                      f"steps), {t_cpu:.1f} s, oracle/gg_oracle.c gcc -O2 single thread (the reference's deterministic thread_count=1)",
            "host_cores_available": os.cpu_count(),
        }
        # the same thread on WARM maps (the steady state of a drive: the map keeps its terrain from cloud to cloud; the cold CPU
        # path is three times slower because every road return of a fresh map starts a line-of-sight walk, :243-275, that the
        # HIP path skips with a host-side flag -- so the like-for-like ratio is warm / warm)
        donew, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < max(3.0, args.cpu_seconds / 3):
            for b in range(n_cpu):
                maps[b].filter_cloud(clouds[(b + donew) % n_cpu], (0.0, 0.0, 0.0), -1.73)
            donew += n_cpu
        tw = time.perf_counter() - t0
        result["cpu_baseline_warm"] = {"value": round(donew / tw, 2), "unit": "clouds/s", "cores": 1, "kind": "port",
                                       "sample": f"{donew} calls, {tw:.1f} s, maps kept from call to call"}
        result["speedup_vs_cpu_1thread"] = {
            "cold_over_cold": round(value / (done / t_cpu), 1),
            "warm_over_warm": round(result["warm_map"]["clouds_per_s"] / (donew / tw), 1),
            "note": "the >= 10x target of the north star is judged on warm_over_warm (like for like: on a fresh map the CPU path walks a "
                    "line of sight for every road return and the HIP path provably need not); a reported ratio, not a kernel-quality figure",
        }
        done8, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < max(3.0, args.cpu_seconds / 3):
            for b in range(n_cpu):
                maps[b].reset_state()
                maps[b].filter_cloud_threads(clouds[b], (0.0, 0.0, 0.0), -1.73, 8)
            done8 += n_cpu
        t8 = time.perf_counter() - t0
        result["cpu_baseline_8p4"] = {
            "value": round(done8 / t8, 2), "unit": "clouds/s", "cores": 8, "kind": "port",
            "sample": f"{done8} calls, {t8:.1f} s: the reference's default threading shape (8 racing insertion threads + 4 detection "
                      "threads, cfg/GroundGrid.cfg:21, src/GroundSegmentation.cpp:98-134) -- timing only, not deterministic",
        }

        # the drop-in call: gg_filter_cloud with host buffers in and out (PCIe both ways), one map, a stream of clouds
        chk = api.GroundSegmentation().init(120.0, 0.33, n_slots=1, max_points=stride, device=local_rank)
        seq = [clouds[b % min(B, 8)] for b in range(64)]
        for c in seq[:4]:
            chk.filter_cloud(c, (0.0, 0.0, 0.0), -1.73)
        t_sync = t_pipe = t_bind = t_bind_pin = t_dev = t_pc2 = t_two = float("inf")
        layer_buf = chk.alloc_layers(register=False)   # the planes of a host grid_map::GridMap: allocated once, written per cloud
        layer_pin = chk.alloc_layers(register=True)    # ... and registered with the context (what ros/GroundGridHip.cpp does for the map it owns)
        wire_seq = [api.to_pc2(c).tobytes() for c in seq[:8]]
        for _rep in range(3):  # best of three passes (the leg is host-bound: page placement and clocks of the box vary)
            t0 = time.perf_counter()
            for c in seq:
                chk.filter_cloud(c, (0.0, 0.0, 0.0), -1.73, reuse_buffers=True)
            t_sync = min(t_sync, (time.perf_counter() - t0) / len(seq))
            t0 = time.perf_counter()
            tick = chk.filter_cloud_async(seq[0], (0.0, 0.0, 0.0), -1.73)
            for k in range(len(seq)):
                nxt = chk.filter_cloud_async(seq[k + 1], (0.0, 0.0, 0.0), -1.73) if k + 1 < len(seq) else None
                chk.filter_cloud_wait(tick, reuse_buffers=True)
                tick = nxt
            t_pipe = min(t_pipe, (time.perf_counter() - t0) / len(seq))
            t0 = time.perf_counter()
            for c in seq[:32]:  # what the reference-typed binding does per callback (GROUNDGRID_HIP_LAYERS=all): one fused call
                chk.filter_cloud_with_layers(c, (0.0, 0.0, 0.0), -1.73, layer_buf, reuse_buffers=True)
            t_bind = min(t_bind, (time.perf_counter() - t0) / 32)
            t0 = time.perf_counter()
            for c in seq[:32]:
                chk.filter_cloud_with_layers(c, (0.0, 0.0, 0.0), -1.73, layer_pin, reuse_buffers=True)
            t_bind_pin = min(t_bind_pin, (time.perf_counter() - t0) / 32)
            t0 = time.perf_counter()
            for c in seq[:32]:  # the round-4 shape of the same thing: two calls, the layers after the cloud
                chk.filter_cloud(c, (0.0, 0.0, 0.0), -1.73, reuse_buffers=True)
                chk.map(0).layers()
            t_two = min(t_two, (time.perf_counter() - t0) / 32)
            t0 = time.perf_counter()
            for k in range(32):  # wire to wire: 18-byte PointCloud2 payload in, 18-byte records of the returned cloud out
                chk.filter_cloud_pc2_out(wire_seq[k % 8], len(seq[k % 8]), 18, (0, 4, 8, 16), (0.0, 0.0, 0.0), -1.73)
            t_pc2 = min(t_pc2, (time.perf_counter() - t0) / 32)
            # the device-resident binding (groundgrid_amd/host/ros/GroundGridHip.cpp + GroundSegmentationHip.cpp): GroundGrid::update
            # runs on the device before every cloud (the map scrolls by a cell per frame: a moving vehicle), nothing is uploaded and
            # no layer is downloaded (no subscriber)
            m0 = chk.map(0)
            t0 = time.perf_counter()
            for k, c in enumerate(seq):
                m0.move(0.4 * (k % 2), 0.0, (-0.4 * (k % 2), 0.0, 1.73, 0.0, 0.0, 0.0, 1.0))
                chk.filter_cloud(c, (0.0, 0.0, 0.0), -1.73, reuse_buffers=True)
            t_dev = min(t_dev, (time.perf_counter() - t0) / len(seq))
            m0.move(0.0, 0.0, (0.0, 0.0, 1.73, 0.0, 0.0, 0.0, 1.0))
        cpu_warm = donew / tw
        result["host_api"] = {
            "sync_clouds_per_s": round(1.0 / t_sync, 1), "pipelined_clouds_per_s": round(1.0 / t_pipe, 1),
            "binding_like_clouds_per_s": round(1.0 / t_bind, 1), "device_resident_binding_clouds_per_s": round(1.0 / t_dev, 1),
            "binding_like_registered_clouds_per_s": round(1.0 / t_bind_pin, 1), "binding_like_two_calls_clouds_per_s": round(1.0 / t_two, 1),
            "pc2_out_clouds_per_s": round(1.0 / t_pc2, 1),
            "sync_ms": round(1e3 * t_sync, 4), "pipelined_ms": round(1e3 * t_pipe, 4), "binding_like_ms": round(1e3 * t_bind, 4),
            "binding_like_registered_ms": round(1e3 * t_bind_pin, 4), "binding_like_two_calls_ms": round(1e3 * t_two, 4), "pc2_out_ms": round(1e3 * t_pc2, 4),
            "device_resident_binding_ms": round(1e3 * t_dev, 4),
            "vs_cpu_1thread": round((1.0 / t_pipe) / cpu_warm, 1),  # (consecutive clouds on one map: the warm CPU figure)
            "sync_vs_cpu_1thread": round((1.0 / t_sync) / cpu_warm, 1),
            "binding_like_vs_cpu_1thread": round((1.0 / t_bind) / cpu_warm, 1),
            "binding_like_registered_vs_cpu_1thread": round((1.0 / t_bind_pin) / cpu_warm, 1),
            "pc2_out_vs_cpu_1thread": round((1.0 / t_pc2) / cpu_warm, 1),
            "device_resident_binding_vs_cpu_1thread": round((1.0 / t_dev) / cpu_warm, 1),
            "note": "gg_filter_cloud: 32-byte PointXYZIR cloud in host memory -> returned cloud in host memory, one map, consecutive clouds; "
                    "pipelined = gg_filter_cloud_async two clouds deep (pack + upload of cloud k+1 overlap the kernels of cloud k); binding_like = "
                    "gg_filter_cloud_layers with all 11 layers into plain host planes (what groundgrid_amd/host/ros/GroundSegmentationHip.cpp does "
                    "per callback when the map is host-managed and every layer is published: the layers the insertion finishes travel while the "
                    "sweep runs); binding_like_registered = the same into planes registered with gg_host_register (the device writes them, no "
                    "staging copy); binding_like_two_calls = round 4's shape, gg_filter_cloud then gg_get_layers; pc2_out = gg_filter_cloud_pc2_out, "
                    "18-byte PointCloud2 payload in and 18-byte records of the returned cloud out (the label kernel writes them); device_resident_binding = the same call with "
                    "GroundGrid::update on the device before every cloud (gg_move_map, the map scrolls a cell per frame) and no layer downloaded: "
                    "what the pair ros/GroundGridHip.cpp + ros/GroundSegmentationHip.cpp does per callback; 64 clouds of 8 different scenes in "
                    "turn, best of three passes",
        }
        chk.release_layers(layer_pin)
        del layer_buf, layer_pin

        # single-cloud latency through the same kernels (one cloud per launch, device-resident input): the captured graph, then the
        # eager launches with an event pair around every kernel (where the time goes; the events cost a little themselves)
        p1 = points[:1].contiguous()
        o1 = None
        side = torch.cuda.Stream(device=dev)  # (graphs are captured on a real stream, not the legacy default one)
        with torch.cuda.stream(side):
            for _ in range(5):
                o1 = chk.filter_batch(p1, n_points[:1], origins[:1], base_z[:1], out=o1)
            chk.synchronize()
            t1 = time.perf_counter()
            for _ in range(40):
                o1 = chk.filter_batch(p1, n_points[:1], origins[:1], base_z[:1], out=o1)
            chk.synchronize()
            result["single_cloud_latency_ms"] = round((time.perf_counter() - t1) / 40 * 1e3, 4)
            chk.debug_set_tuning("graphs", 1)  # the same 40 calls as replays of a captured HIP graph (opt-in, GG_GRAPH=1)
            for _ in range(5):
                o1 = chk.filter_batch(p1, n_points[:1], origins[:1], base_z[:1], out=o1)
            chk.synchronize()
            t1 = time.perf_counter()
            for _ in range(40):
                o1 = chk.filter_batch(p1, n_points[:1], origins[:1], base_z[:1], out=o1)
            chk.synchronize()
            result["single_cloud_latency_graph_replay_ms"] = round((time.perf_counter() - t1) / 40 * 1e3, 4)
            result["single_cloud_graph_replays"] = chk.debug_set_tuning("graph_replays", 0)
            chk.debug_set_tuning("graphs", 0)
            chk.set_flags(profile=True)
            for _ in range(5):
                o1 = chk.filter_batch(p1, n_points[:1], origins[:1], base_z[:1], out=o1)
            chk.synchronize()
            chk.kernel_times(reset=True)
            t1 = time.perf_counter()
            for _ in range(20):
                o1 = chk.filter_batch(p1, n_points[:1], origins[:1], base_z[:1], out=o1)
            chk.synchronize()
            result["single_cloud_latency_eager_profiled_ms"] = round((time.perf_counter() - t1) / 20 * 1e3, 4)
            result["single_cloud_kernel_ms"] = {k: round(v[0] / max(1, v[1]), 4) for k, v in chk.kernel_times(reset=True).items()}
        chk.close()

        # BASELINE configs[3]: dense OS-128-style clouds, 200 m / 0.2 m -> 1000 x 1000 cells
        try:
            result["config4"] = config4_leg(args, api, torch, dev, local_rank, seg, Pipeline, check_timed_outputs, to_device)
        except Exception as e:  # the headline must not depend on the stress configuration
            result["config4"] = {"error": repr(e)}

        # BASELINE configs[4]'s shape on synthetic data: thousands of consecutive full-size frames, the map scrolling in every one
        if args.drive_frames > 0:
            try:
                seg.close()  # (the headline context's 12 GB are not needed any more)
                result["config5_synthetic"] = drive_leg(args, local_rank)
            except Exception as e:
                result["config5_synthetic"] = {"error": repr(e)}

    if rank == 0 and world == 1 and args.only_config4:
        from oracle import oracle  # noqa: F401  (config4_leg checks its timed outputs)

        result["config4"] = config4_leg(args, api, torch, dev, local_rank, seg, Pipeline, check_timed_outputs, to_device)
    if rank == 0:
        print(json.dumps(ordered_line(result, world)))
    if dist:
        dist.barrier()
        dist.destroy_process_group()


def config4_leg(args, api, torch, dev, local_rank, seg_main, Pipeline, check_timed_outputs, to_device):
    """BASELINE configs[3] at a GPU-filling batch (the batched fraction) and as single-cloud latency."""
    from groundgrid_amd import synth
    from oracle import oracle

    seg_main.close()  # frees the headline's 12 GB arena
    torch.cuda.empty_cache()
    B4 = max(1, args.config4_batch)
    base4 = synth.os128_cloud_fast(seed=20240113)  # ~2.1 M returns; the other clouds of the batch are yaw rotations of it

    class Rotations:
        """cloud b = the base cloud rotated by 2 pi b / B4 about z -- regenerated on demand (128 clouds of 67 MB each are not
        kept in host memory: the device holds the packed records, the checks re-make the few clouds they look at)."""

        def __len__(self):
            return B4

        def __getitem__(self, b):
            if b == 0:
                return base4
            ang = np.float32(2.0 * np.pi * b / B4)
            cc, ss = np.cos(ang), np.sin(ang)
            o = synth.clone_cloud(base4)
            o["x"] = (cc * base4["x"] - ss * base4["y"]).astype(np.float32)
            o["y"] = (ss * base4["x"] + cc * base4["y"]).astype(np.float32)
            return o

    c4 = Rotations()
    n4 = [len(base4)] * B4
    s4 = (len(base4) + 63) // 64 * 64
    seg4 = api.GroundSegmentation().init(200.0, 0.2, n_slots=B4, max_points=s4, device=local_rank)
    seg4.set_flags(profile=True)
    p4 = torch.zeros((B4, s4, 16), dtype=torch.uint8, device=dev)
    for b in range(B4):
        p4[b, : n4[b]] = torch.from_numpy(api.pack16(c4[b]).view(np.uint8).reshape(-1, 16)).to(dev)
    pipe4 = Pipeline(seg4, p4, n4, np.zeros((B4, 3), np.float32), np.full(B4, -1.73), cold=True)
    steps4 = 4
    e4, kt4 = pipe4.timed(steps4, 2)
    cnt4 = pipe4.out.counts.cpu().numpy()
    C4, T4 = seg4.rows * seg4.rows, ((seg4.rows + 15) // 16) ** 2
    alg4 = algorithmic_bytes(float(np.mean(n4)), float(np.mean(cnt4[:, 1] + cnt4[:, 2] + cnt4[:, 3])), float(np.mean(cnt4[:, 1])), C4, T4,
                             (s4 + seg4.debug_set_tuning("pw", 0) - 1) // seg4.debug_set_tuning("pw", 0))
    tab4 = kernel_table(kt4, alg4, B4)
    step_real4 = add_real_traffic(tab4, B4, section="config4_kernels")
    dom4 = max(tab4, key=lambda k: tab4[k]["avg_ms"])
    ins4 = sum(tab4[k]["avg_ms"] for k in ("k_classify", "k_scan", "k_scatter", "k_reduce") if k in tab4)
    ok4, chk4 = check_timed_outputs(pipe4, c4, 200.0, 0.2, n_check=min(4, B4), seed=4)
    m4 = oracle.OracleMap(200.0, 0.2)
    t0 = time.perf_counter()
    n_cpu4 = 0
    cpu_clouds4 = [c4[0], c4[1 % B4]]  # (two of the batch's clouds in turn: making a rotated 67 MB cloud is not what is timed)
    while n_cpu4 < 30 and (time.perf_counter() - t0 < 12.0 or n_cpu4 < 8):  # >= 30 calls (~0.3 s each) unless the host is very slow
        m4.reset_state()
        m4.filter_cloud(cpu_clouds4[n_cpu4 % 2], (0.0, 0.0, 0.0), -1.73)
        n_cpu4 += 1
    t4 = (time.perf_counter() - t0) / n_cpu4
    out = {
        "workload": f"BASELINE configs[3]: {int(np.mean(n4))} points per cloud (128 rings x 16384 azimuths), 1000x1000 grid @ 0.2 m, "
                    f"{B4} clouds per launch (rotating over the slots), cold maps",
        "clouds_per_s": round(B4 * steps4 / e4, 2), "ms_per_step": round(1e3 * e4 / steps4, 4), "ms_per_cloud": round(1e3 * e4 / steps4 / B4, 4),
        "roofline": {"kernel": dom4, "bound": "hbm", "achieved": tab4[dom4]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": tab4[dom4]["frac_hbm"], "traffic": pmc_traffic(dom4, B4, "config4_kernels"), "real_frac": tab4[dom4].get("real_frac_hbm"),
                     "traffic_ratio": tab4[dom4].get("traffic_ratio")},
        "step_real_frac_hbm": step_real4,
        "kernels": tab4,
        "all_kernels_frac_hbm": round(sum(alg4.values()) * B4 / (1e-3 * sum(r["avg_ms"] for r in tab4.values())) / 1e9 / HBM_PEAK_GBS, 4),
        "scatter_read_frac": round(20.0 * float(np.mean(n4)) * B4 / (ins4 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "cpu_baseline": {"value": round(1.0 / t4, 3), "unit": "clouds/s", "cores": 1, "kind": "port", "sample": f"{n_cpu4} calls, cold maps, {t4 * n_cpu4:.2f} s"},
        "parity_checked_in_run": ok4, "parity_sampled": chk4,
    }
    # one cloud per launch: the latency a single dense sensor would see (device-resident input)
    p1 = p4[:1].contiguous()
    del p4
    pipe1 = Pipeline(seg4, p1, n4[:1], np.zeros((1, 3), np.float32), np.full(1, -1.73), cold=True)
    e1, kt1 = pipe1.timed(10, 3)
    ok1, _ = check_timed_outputs(pipe1, [base4], 200.0, 0.2, n_check=1, seed=5)
    out["single_cloud"] = {"latency_ms": round(1e3 * e1 / 10, 4), "kernel_ms": {k: round(v[0] / max(1, v[1]), 4) for k, v in kt1.items()},
                           "parity_checked_in_run": ok1}
    seg4.close()
    return out


class _OracleBackend:
    """The CPU path behind the replay harness (groundgrid_amd.replay): the checker and the CPU baseline of the drive leg."""

    def __init__(self):
        self.m = None

    def reset(self, pos, odom_z):
        from oracle import oracle

        self.m = oracle.OracleMap(120.0, 0.33, pos=pos, odom_z=float(odom_z))

    def move(self, odom, base_to_map):
        self.m.update(odom[0], odom[1], base_to_map)

    def filter(self, cloud_map, origin, base_z):
        r = self.m.filter_cloud(cloud_map, origin, base_z)
        return r["label"], r["index"]


def drive_leg(args, local_rank):
    """BASELINE configs[4]'s SHAPE (SemanticKITTI sequence 00: 4540 consecutive clouds on ONE map that scrolls with the vehicle, the
    evaluator's table at the end) on synthetic data -- the dataset is not in the image: groundgrid_amd.kitti.synthetic_drive, a closed
    loop of 0.8 m per frame through eight seeded HDL-64E scenes, wired like a sequence directory.  Per frame GroundGrid::update on the
    device (gg_move_map) and one synchronous gg_filter_cloud, host buffers both ways; the CPU path (the oracle, one thread) runs the same
    frames side by side: labels and returned-cloud order compared in EVERY frame, ground / groundpatch after the LAST one (what decays
    and scrolls for thousands of frames), the two evaluator tables against each other."""
    import numpy as np

    from groundgrid_amd import kitti, replay

    n = args.drive_frames
    dev_b, cpu_b = replay.DeviceBackend(device=local_rank, max_points=140000), _OracleBackend()
    t0 = time.perf_counter()
    ev, t_dev, t_cpu, n_cpu, same, first_bad = replay.replay_side_by_side(kitti.synthetic_drive(n), dev_b, cpu_b)
    wall = time.perf_counter() - t0
    final_same = True
    for name in ("ground", "groundpatch"):
        a, b = dev_b.map.get(name), cpu_b.m.layer(name)
        final_same = final_same and bool(np.array_equal(a, b, equal_nan=True))
    out = {
        "workload": f"BASELINE configs[4] shape, synthetic: {n} consecutive ~125 k-point HDL-64E clouds (8 seeded scenes in turn) along a closed loop of "
                    f"{0.8 * n / 1000.0:.2f} km, one 364 x 364 map scrolled by GroundGrid::update on the device every frame; SemanticKITTI itself is not in the image",
        "frames": n, "clouds_per_s": round(n / t_dev, 1), "ms_per_frame": round(1e3 * t_dev / n, 4),
        "call": "gg_move_map + synchronous gg_filter_cloud (host buffers both ways) per frame", "seconds_wall_incl_frame_synthesis_and_cpu": round(wall, 1),
        "cpu_baseline": {"value": round(n_cpu / t_cpu, 1) if t_cpu > 0 else None, "unit": "clouds/s", "cores": 1, "kind": "port",
                         "sample": f"the same {n_cpu} frames, GroundGrid::update + filter_cloud per frame, {t_cpu:.1f} s"},
        "labels_and_order_identical_in_every_frame": bool(same), "first_frame_that_differed": first_bad, "final_map_identical": bool(final_same),
        "map_position_after_the_loop": [round(float(v), 3) for v in dev_b.map.getPosition()], "evaluator": ev.rows(),
        "parity_checked_in_run": bool(same and final_same),
    }
    print(ev.table(), file=sys.stderr)
    dev_b.seg.close()
    return out


def kitti_leg(args, local_rank):
    """BASELINE configs[0] / configs[4]: replay a SemanticKITTI sequence on one GPU (device-resident map scroll), print clouds/s
    and the evaluator's per-label table, and diff it against the reference's published sequence-00 table
    (tests/golden/readme_seq00_table.json = /root/reference/README.md:57-94; a close-match target: the ROS pipeline's tf timing
    is not part of the data)."""
    from groundgrid_amd import kitti, replay

    seq = kitti.KittiSequence(args.kitti_dir, euler_roundtrip=args.kitti_euler_roundtrip)
    n = len(seq) if not args.kitti_max_frames else min(len(seq), args.kitti_max_frames)
    t0 = time.perf_counter()
    ev, spent = replay.replay((seq.frame(i) for i in range(n)), replay.DeviceBackend(device=local_rank))
    wall = time.perf_counter() - t0
    result = {
        "metric": "point clouds/s (SemanticKITTI sequence replay, one map, consecutive clouds)", "value": round(n / spent, 2), "unit": "clouds/s",
        "n_gpus": 1, "clouds": n, "seconds_in_device_path": round(spent, 3), "seconds_wall_incl_io": round(wall, 3),
        "data": f"SemanticKITTI-format sequence at {args.kitti_dir}", "higher_is_better": True,
        "table": ev.rows(),
    }
    golden = os.path.join(ROOT, "tests", "golden", "readme_seq00_table.json")
    if os.path.exists(golden):
        result["vs_readme_seq00"] = ev.compare_with(json.load(open(golden)), tolerance_pct=1.0)
    print(ev.table(), file=sys.stderr)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
