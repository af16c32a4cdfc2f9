#!/usr/bin/env python3
"""gg_fuse_states on the headline shape of tools/bench_visibility.py (1024 maps of 364 x 364, the observation planes those of
visibility_clouds on 1024 GG_POINT16 clouds of a 64-ring scan, the prior the evidence of an earlier call, a non-zero index shift), timed by
stream events, median of --reps with the warm-up excluded; ms per 1024 maps:

  fuse_all        (a) fuse_states with every output: evidence, fused state, frontier, counts
  fuse_evidence   (b) ... the evidence alone
  torch           (c) the torch composition of the same planes on the same device: a shifted copy into a zeroed buffer, clamp, where, clamp,
                  two thresholds, an eight-neighbour max-pool (float16) for the frontier, four sums for the counts.  Its four results are
                  asserted bit-equal to (a)'s before anything is timed.  Every map gets THE SAME shift, so that the shifted copy is one
                  slice assignment for the whole batch -- the most favourable case for torch; with a shift per map it needs a gather or
                  a copy per map
  copy            (d) one device-to-device copy that moves as many bytes as (a)'s algorithmic traffic (it reads half of them and writes
                  half): the bandwidth yardstick of this session

Every repetition runs (a) (c) (a) (c) (b) (d); the two A/B pairs are reported apart.  Needs a GPU; writes one JSON file and prints it.  For
times per kernel run the tool alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_fusion.py --reps 3`.

    python tools/bench_fusion.py --out profiles/fusion/summary.json
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

# the defaults of GroundSegmentation.fuse_states but decay = 1 (the decay step is then not a no-op).  With a miss and a decay per frame no
# cell of this workload reaches free_threshold; what the kernel loads and stores does not depend on the values
PARAMS = dict(hit=4, miss=1, decay=1, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)


def torch_fusion(torch, states, prior, shift, p, scratch):
    """what a caller composes today; returns (evidence, fused, frontier, counts)"""
    B, R, Cc = states.shape
    s0, s1 = shift
    P = scratch
    P.zero_()
    r0, r1, c0, c1 = max(0, -s0), min(R, R - s0), max(0, -s1), min(Cc, Cc - s1)
    if r0 < r1 and c0 < c1:
        P[:, r0:r1, c0:c1] = prior[:, r0 + s0: r1 + s0, c0 + s1: c1 + s1]
    P.clamp_(p["e_min"], p["e_max"])
    D = torch.where(P > 0, (P - p["decay"]).clamp_min_(0), (P + p["decay"]).clamp_max_(0))
    E = (D + torch.where(states > 0, p["hit"], torch.where(states < 0, -p["miss"], 0))).clamp_(p["e_min"], p["e_max"]).to(torch.int32)
    F = torch.where(E >= p["occ_threshold"], 1, torch.where(E <= p["free_threshold"], -1, 0)).to(torch.int32)
    near = torch.nn.functional.max_pool2d((F == 0).to(torch.float16)[:, None], 3, 1, 1)[:, 0] > 0
    frontier = torch.where((F == -1) & near, 0, -1).to(torch.int32)
    counts = torch.stack([(F == -1).sum((1, 2)), (F == 0).sum((1, 2)), (F == 1).sum((1, 2)), (frontier == 0).sum((1, 2))], 1).to(torch.int32)
    return E, F, frontier, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--shift", type=int, nargs=2, default=(3, -2))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_fusion.py needs a GPU")
    B, p, shift = args.maps, PARAMS, tuple(args.shift)
    assert shift != (0, 0)
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
    shifts = np.tile(np.array(shift, np.int32), (B, 1))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)  # one default batch
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        # the prior: two earlier frames of the same observations, scrolled against each other
        prior = seg.fuse_states(states, seg.fuse_states(states, on_torch_stream=True, **p).evidence, shifts=-shifts, on_torch_stream=True, **p).evidence
        full = seg.fuse_states(states, prior, shifts=shifts, on_torch_stream=True, **p)
        only = seg.fuse_states(states, prior, shifts=shifts, fused=False, frontier=False, counts=False, on_torch_stream=True, **p)
        scratch = torch.empty_like(prior)
        E, F, frontier, counts = torch_fusion(torch, states, prior, shift, p, scratch)
        stream.synchronize()
        assert torch.equal(E, full.evidence) and torch.equal(F, full.state) and torch.equal(frontier, full.frontier) and torch.equal(counts, full.counts)
        assert torch.equal(only.evidence, full.evidence)
        cnt = full.counts.double().mean(0).tolist()
        traffic = B * rows * cols * 4 * 5  # per cell: state and prior read, evidence, fused and frontier written
        src = torch.empty(traffic // 8, dtype=torch.int32, device="cuda")  # (the copy reads traffic / 2 bytes and writes as many)
        dst = torch.empty_like(src)
        src.zero_()
        del E, F, frontier, counts
        shape = {"maps": B, "rows": rows, "cols": cols, "shift": list(shift), "params": p, "free_cells_per_map": cnt[0], "unknown_cells_per_map": cnt[1],
                 "occupied_cells_per_map": cnt[2], "frontier_cells_per_map": cnt[3], "algorithmic_bytes_fuse_all": traffic, "algorithmic_bytes_fuse_evidence": traffic * 3 // 5,
                 "copy_bytes_read_plus_written": int(src.numel()) * 8}

        def run(what):
            if what.startswith("fuse_all"):
                seg.fuse_states(states, prior, shifts=shifts, out=full, on_torch_stream=True, **p)
            elif what.startswith("torch"):
                torch_fusion(torch, states, prior, shift, p, scratch)
            elif what == "fuse_evidence":
                seg.fuse_states(states, prior, shifts=shifts, fused=False, frontier=False, counts=False, out=only, on_torch_stream=True, **p)
            else:
                dst.copy_(src)

        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in ("fuse_all_1", "torch_1", "fuse_all_2", "torch_2", "fuse_evidence", "copy"):  # A/B/A/B, then the other two
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(what)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()  # (once: the device never idles between repetitions)
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup, "unit": "ms per %d maps" % B, "torch_equals_fuse_all": True}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    a = 0.5 * (results["fuse_all_1"]["ms_median"] + results["fuse_all_2"]["ms_median"])
    results["fuse_all_ms"] = a
    results["fuse_all_faster_than_torch_in_both_pairs"] = bool(results["fuse_all_1"]["ms_median"] < results["torch_1"]["ms_median"]
                                                               and results["fuse_all_2"]["ms_median"] < results["torch_2"]["ms_median"])
    results["ratio_torch_over_fuse_all"] = [results["torch_%d" % k]["ms_median"] / results["fuse_all_%d" % k]["ms_median"] for k in (1, 2)]
    results["ratio_fuse_all_over_copy"] = a / results["copy"]["ms_median"]
    results["fuse_all_GBps_algorithmic"] = traffic / a / 1e6
    results["copy_GBps"] = shape["copy_bytes_read_plus_written"] / results["copy"]["ms_median"] / 1e6
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
