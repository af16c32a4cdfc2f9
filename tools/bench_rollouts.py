#!/usr/bin/env python3
"""gg_score_rollouts on the planes of tools/bench_headings.py (1024 maps of 364 x 364, K = 16): the heading masks of footprint_planes for
that benchmark's car on the fused states of its drive, the D volume of route_headings on those masks (goal cells within 16 cells of the
frontier, w = 1), the squared clearance of clearance_planes on the fused state, and an inflation cost plane made of it
(max(1, 100 - dist2)).  The rollouts are the arc library of api.rollout_arcs: 32 speeds (0.25 .. 2 cells per step) x 64 turn rates
(+-0.12 rad per step) = 2048 arcs of 32 steps, scored from the robot cell (the middle of the map, its centre, heading 0) with reach 0.
Timed by stream events, the arms interleaved round by round in one process, median / min / max of --reps with the warm-up excluded;
ms per call.  The tables are handed over step-major, so no arm times the permuting copy of the Python method.

  all            (a) records and best with mask, cost, dist and clear
  no_clear       (b) as (a) without d_clear
  no_dist        (c) as (a) without d_dist
  per_map_abs    (d) as (a) with a table per map in the absolute frame (the poses (a) visits, so the records are (a)'s on bits: asserted)
  p256, p8192    (e) as (a) with 256 arcs (every eighth) and with 8192 (64 speeds x 128 turn rates)
  one_map        (f) as (a) for n = 1: a single map runs on one compute unit -- a latency, not a target
  copy           (g) one device-to-device copy that moves as many bytes as (a)'s ALGORITHMIC traffic (it reads half and writes half).
                 Counted from (a)'s records: 32 bytes per record and 16 per map written; the shared table once (16 P T); per rollout
                 one mask word per pose tested (min(steps + 1, len)), one cost and one clearance word per admissible pose (steps), one
                 word of D per complete rollout.  The table re-read by every work-group and the sectors around a gathered word are
                 not algorithmic and are not counted
  torch          (h) the caller's alternative on the same device, for records and best that equal (a)'s bit for bit (asserted): the
                 rotation in int64, three gathers, a cumprod of admissibility, masked sums and minima, one gather of D, a min over
                 keys.  Batched over --torch-maps maps per pass (the [maps, steps, rollouts] int64 temporaries of all 1024 would not
                 leave room), on --torch-sample maps, SCALED to all of them

Needs a GPU; writes one JSON file and prints it.  For counters run the tool alone under
`rocprofv3 --pmc ... -- python tools/bench_rollouts.py --reps 2 --torch-sample 0`.

    python tools/bench_rollouts.py --out profiles/rollouts/summary.json
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

FUSE = dict(hit=4, miss=3, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)  # tools/bench_headings.py
CAR = dict(ahead=11.2, behind=3.0, left=2.9, right=2.9)
MOVES = dict(step=2, unit=10, turn=3, reverse_pct=150)
NONE = _lib.GG_ROUTE_NONE
COST_MAX = 252


def torch_poses(table, starts, rot, K):
    """(r16_t, c16_t, k_t, s) int64 [B, T, P] of a shared step-major table [T, P, 4] in the relative frame"""
    import torch

    da, db, dk, s = (table[..., j].long()[None] for j in range(4))
    r16, c16, k0 = (starts[:, j].long().view(-1, 1, 1) for j in range(3))
    cq, sq = rot[k0.view(-1), 0].long().view(-1, 1, 1), rot[k0.view(-1), 1].long().view(-1, 1, 1)
    rha = lambda v: torch.sign(v) * ((v.abs() + 8192) >> 14)
    return r16 + rha(cq * da - sq * db), c16 + rha(sq * da + cq * db), torch.remainder(k0 + dk, K), s.expand(r16.shape[0], -1, -1)


def torch_scores(mask, cost, dist, clear, table, starts, rot, K, rows, cols):
    """records [B, P, 8] and best [B, 4] in torch, bit for bit gg_score_rollouts' for a map with a start, reach 0, a shared relative table"""
    import torch

    B, cells = mask.shape[0], rows * cols
    T, P = table.shape[:2]
    pr, pc, k, s = torch_poses(table, starts, rot, K)
    row, col = pr >> 4, pc >> 4
    inside = (row >= 0) & (row < rows) & (col >= 0) & (col < cols)
    cell = (row.clamp(0, rows - 1) * cols + col.clamp(0, cols - 1)).view(B, -1)
    gather = lambda plane: plane.view(B, -1).gather(1, cell).view(B, T, P).long()
    valid = torch.cumprod((s > 0).long(), dim=1)
    ok = torch.cumprod((inside & (((gather(mask) >> k) & 1) != 0)).long() * valid, dim=1)
    length, steps = valid.sum(1), ok.sum(1)
    total_cost = (torch.clamp(s, max=32767) * gather(cost).clamp(1, COST_MAX) * ok).sum(1)
    low = torch.where(ok != 0, gather(clear), torch.full_like(ok, NONE)).min(dim=1).values
    last = (steps - 1).clamp(min=0).unsqueeze(1)
    start_cell = ((starts[:, 0].long() >> 4) * cols + (starts[:, 1].long() >> 4)).view(B, 1)
    end_cell = torch.where(steps > 0, cell.view(B, T, P).gather(1, last).squeeze(1), start_cell.expand(B, P))
    end_k = torch.where(steps > 0, k.expand(B, T, P).gather(1, last).squeeze(1), starts[:, 2].long().view(B, 1).expand(B, P))
    complete = steps == length
    togo = torch.where(complete, dist.view(B, -1).gather(1, end_k * cells + end_cell).long(), torch.full_like(steps, NONE))
    scored = complete & (togo != NONE) & (togo >= 0)
    total = torch.where(scored, torch.clamp(total_cost + togo, max=NONE - 1), torch.full_like(steps, NONE))
    records = torch.stack([steps, length, total_cost, end_cell, end_k, togo, low, total], dim=2).to(torch.int32)
    key = torch.where(scored, (total << 32) | torch.arange(P, device=mask.device).view(1, P), torch.full_like(total, (1 << 62)))
    least = key.min(dim=1).values
    any_scored = scored.any(dim=1)
    best = torch.stack([torch.where(any_scored, least & 0xFFFFFFFF, torch.full_like(least, -1)), torch.where(any_scored, least >> 32, torch.full_like(least, NONE)),
                        complete.sum(1), scored.sum(1)], dim=1).to(torch.int32)
    return records, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-az", type=int, default=300)
    ap.add_argument("--goal-reach", type=int, default=16)
    ap.add_argument("--torch-maps", type=int, default=32, help="maps per pass of the torch composition")
    ap.add_argument("--torch-sample", type=int, default=128, help="maps the torch composition runs on (0: skip it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_rollouts.py needs a GPU")
    B, K, T = args.maps, 16, 32
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
    shifts = np.tile(np.array((3, -2), np.int32), (B, 1))
    rot = api.rotation_table(2.0 * np.pi * np.arange(K) / K)
    moves = api.heading_moves(rot, **MOVES)
    arcs = {2048: api.rollout_arcs(rot, np.linspace(0.25, 2.0, 32), np.linspace(-0.12, 0.12, 64), T),
            8192: api.rollout_arcs(rot, np.linspace(0.25, 2.0, 64), np.linspace(-0.12, 0.12, 128), T)}
    arcs[256] = arcs[2048][::8]
    starts = np.tile(np.array((16 * (rows // 2) + 8, 16 * (cols // 2) + 8, 0), np.int32), (B, 1))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        seg.reset_maps(0, B, odom_z=0.0, on_torch_stream=True)
        batch = seg.filter_batch(pts, n_pts, origins, base_z)
        seg.batch_fence()
        states = seg.visibility_clouds(pts, n_pts, origins, labels=batch.labels, min_points=2, min_height=0.3, max_height=2.5).state
        first = seg.fuse_states(states, on_torch_stream=True, **FUSE)
        second = seg.fuse_states(states, first.evidence, shifts=-shifts, on_torch_stream=True, **FUSE)
        fused = seg.fuse_states(states, second.evidence, shifts=shifts, on_torch_stream=True, **FUSE)
        near = seg.clearance_planes(fused.frontier, nearest=False, distance=False, on_torch_stream=True)
        goals = torch.where(near.dist2 <= args.goal_reach ** 2, 0, -1).to(torch.int32).contiguous()
        mask = seg.footprint_planes(fused.state, api.footprint_spans(rot, **CAR, radius=14), min_fit=1, fit=False, counts=False, on_torch_stream=True).mask
        dist = seg.route_headings(mask, goals, moves, cost_max=1, next=False, best=False, counts=False, on_torch_stream=True).dist
        occupied = torch.where(fused.state == _lib.GG_CELL_OCCUPIED, 0, -1).to(torch.int32).contiguous()
        clear = seg.clearance_planes(occupied, nearest=False, distance=False, on_torch_stream=True).dist2
        cost = torch.clamp(100 - clear, min=1).to(torch.int32).contiguous()
        del first, second, near, goals, states, batch
        d_starts, d_rot = torch.from_numpy(starts).cuda(), torch.from_numpy(rot).cuda()
        major = {P: torch.from_numpy(np.ascontiguousarray(a.transpose(1, 0, 2))).cuda() for P, a in arcs.items()}  # [T, P, 4]
        full = dict(rotations=rot, cost=cost, dist=dist, clear=clear, cost_max=COST_MAX, step_major=True, on_torch_stream=True)
        outs = {"all": seg.score_rollouts(mask, major[2048], starts, **full),
                "no_clear": seg.score_rollouts(mask, major[2048], starts, **dict(full, clear=None)),
                "no_dist": seg.score_rollouts(mask, major[2048], starts, **dict(full, dist=None)),
                "p256": seg.score_rollouts(mask, major[256], starts, **full),
                "p8192": seg.score_rollouts(mask, major[8192], starts, **full),
                "one_map": seg.score_rollouts(mask[:1], major[2048], starts[:1], **dict(full, cost=cost[:1], dist=dist[:1], clear=clear[:1]))}
        # the per-map absolute tables: the poses the shared relative table visits from every map's start (all starts are equal here, so one
        # map's poses are repeated; the call still reads a table per map)
        pr, pc, pk, ps = torch_poses(major[2048], d_starts[:1], d_rot, K)
        per_map = torch.stack([pr, pc, pk, ps], dim=3).to(torch.int32).expand(B, T, 2048, 4).contiguous()
        abs_kw = dict(full, rotations=None, relative=False)
        outs["per_map_abs"] = seg.score_rollouts(mask, per_map, starts, **abs_kw)
        stream.synchronize()
        assert torch.equal(outs["per_map_abs"].records, outs["all"].records) and torch.equal(outs["per_map_abs"].best, outs["all"].best)
        assert torch.equal(outs["one_map"].records[0], outs["all"].records[0])
        rec = outs["all"].records.long()
        steps, length = rec[..., 0], rec[..., 1]
        complete = steps == length
        tested = torch.minimum(steps + 1, length)
        P = 2048
        traffic = int(B * P * 32 + B * 16 + 16 * P * T + 4 * int(tested.sum().item()) + 8 * int(steps.sum().item()) + 4 * int(complete.sum().item()))
        traffic -= traffic % 8
        src = torch.zeros(traffic // 8, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        best = outs["all"].best.double()
        shape = {"maps": B, "rows": rows, "cols": cols, "headings": K, "rollouts": P, "steps": T, "cost_max": COST_MAX, "reach": 0, "fuse_params": FUSE, "car": CAR,
                 "moves": MOVES, "steps_mean": float(steps.double().mean().item()), "complete_per_map": float(best[:, 2].mean().item()),
                 "scored_per_map": float(best[:, 3].mean().item()), "maps_with_a_best": int((outs["all"].best[:, 0] >= 0).sum().item()),
                 "poses_tested": int(tested.sum().item()), "algorithmic_bytes_all": traffic, "table_bytes_shared": 16 * P * T,
                 "table_bytes_if_read_per_map": 16 * P * T * B, "record_bytes": B * P * 32}
        assert shape["steps_mean"] > 1.0, "the scene admits no pose: nothing is measured"

        # the torch composition on a sample of maps, held to the call's records on bits
        sample = min(args.torch_sample, B)
        chunk = max(1, min(args.torch_maps, sample))

        def torch_pass(lo):
            hi = min(lo + chunk, sample)
            return torch_scores(mask[lo:hi], cost[lo:hi], dist[lo:hi], clear[lo:hi], major[2048], d_starts[lo:hi], d_rot, K, rows, cols)

        for lo in range(0, sample, chunk):
            r, b = torch_pass(lo)
            assert torch.equal(r, outs["all"].records[lo: lo + chunk]), f"maps {lo}..: the torch composition and score_rollouts differ in the records"
            assert torch.equal(b, outs["all"].best[lo: lo + chunk]), f"maps {lo}..: the torch composition and score_rollouts differ in best"
            del r, b

        def run(what):
            if what == "copy":
                dst.copy_(src)
            elif what == "torch":
                for lo in range(0, sample, chunk):
                    torch_pass(lo)
            elif what == "per_map_abs":
                seg.score_rollouts(mask, per_map, starts, out=outs[what], **abs_kw)
            elif what == "one_map":
                seg.score_rollouts(mask[:1], major[2048], starts[:1], out=outs[what], **dict(full, cost=cost[:1], dist=dist[:1], clear=clear[:1]))
            else:
                kw = dict(full, clear=None) if what == "no_clear" else dict(full, dist=None) if what == "no_dist" else full
                seg.score_rollouts(mask, major[{"p256": 256, "p8192": 8192}.get(what, 2048)], starts, out=outs[what], **kw)

        arms = ["all", "no_clear", "no_dist", "per_map_abs", "p256", "p8192", "one_map", "copy"] + (["torch"] if sample else [])
        events = {}
        for rep in range(-args.warmup, args.reps):
            for what in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(what)
                e1.record()
                if rep >= 0:
                    events.setdefault(what, []).append((e0, e1))
        stream.synchronize()
    results = {"shape": shape, "reps": args.reps, "warmup": args.warmup, "unit": "ms per call"}
    for what, ev in events.items():
        t = np.array([a.elapsed_time(b) for a, b in ev])
        results[what] = {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}
    ms = lambda what: results[what]["ms_median"]
    results["copy_GBps"] = traffic / ms("copy") / 1e6
    results["all_algorithmic_GBps"] = traffic / ms("all") / 1e6
    results["ratio_all_over_copy"] = ms("all") / ms("copy")
    results["all_us_per_map"] = ms("all") * 1e3 / B
    results["all_ns_per_pose_tested"] = ms("all") * 1e6 / shape["poses_tested"]
    results["ratio_no_clear_over_all"] = ms("no_clear") / ms("all")
    results["ratio_no_dist_over_all"] = ms("no_dist") / ms("all")
    results["ratio_per_map_abs_over_all"] = ms("per_map_abs") / ms("all")
    if sample:
        results["torch"].update({"maps": sample, "maps_per_pass": chunk, "scaled": True, "ms_scaled_to_all_maps": ms("torch") * B / sample, "equals_all_on_bits": True})
        results["ratio_torch_scaled_over_all"] = results["torch"]["ms_scaled_to_all_maps"] / ms("all")
    seg.close()
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
