"""The six calls on caller-held planes in the sequence harness of tests/seq_model.py: gg_fuse_states, gg_route_planes, gg_match_planes,
gg_footprint_planes, gg_route_headings and gg_track_clusters as op kinds (PLANE_KINDS) -- their generator stream, their part of the model
and their part of the driver.  seq_model.py calls into this file; nothing here needs a GPU to import.

They read and write no map state, so their ARITHMETIC cannot depend on the calls around them.  Their ORDERING does: all six run in the frame
of the other many-map calls (one ring of parameter entries, the context's batch and map events), and what they read is what an earlier call
of the sequence -- often on another stream, with nothing but the library between the two -- wrote into a buffer the caller holds.

  input        every plane an op reads is CHAINED, {"op": index, "out": name, "row0": r}: the device buffer that the op at that index of the
               list wrote, from its map r on, as it stands (that op's stride, padding and order), or FOREIGN, {"seed", "kind", "distinct"}:
               seeded words that belong to no call (foreign_plane), of either sign and of large magnitude where the header says that only
               the sign or a clamp counts.
  chain        a list of slots with the caller-held state that goes with them: two evidence buffers used alternately, the id plane of the
               last gg_cluster_clouds, two record and head buffers used alternately.  It outlives checkpoints.  Its shifts are, per slot,
               the sum of what every move of that slot returned since the chain's previous observation ({"since": index, "of": slots}):
               the driver sums what the library returned, the model what its own _move gave.  A reset or set_position of one of its
               slots ends it: the next call has no prior, and names what it lost ("lost") for the mutant that lets a prior survive.
               A chain buffer is written at most once between two checkpoints, so that every output can be compared there.
  map i        of a plane call is row i of its buffers; for the predicates of the coverage table the call "names" slots 0 .. n - 1
               (check_slot_list(ctx, who, n, nullptr, 0) in gg_context.hip fills the call's frame from those slots' flags).

What the model relies on across streams (include/groundgrid_hip.h, "ORDER OF THE MANY-MAP CALLS" at gg_state_fusion and the five other
structures): a many-map call starts after every earlier many-map call of the context has finished, whatever their streams, so a plane that
an earlier call wrote may be read, and a buffer that an earlier call read may be written, with no event of the caller's between the two.
The driver therefore puts its own fills and uploads on the stream of the op they belong to and never refills a chain buffer.
"""
from __future__ import annotations

import json

import numpy as np

from tests import footprint_ref, fusion_ref, headings_ref, match_ref, route_ref, tracks_ref

PLANE_KINDS = ["fuse_states", "route_planes", "match_planes", "footprint_planes", "route_headings", "track_clusters"]
SHIFTED_KINDS = ("fuse_states", "match_planes", "track_clusters")
# the chains the header names: (kind, input) -> the outputs it is chained to somewhere in the committed sequences
CHAIN_TABLE = {
    ("fuse_states", "state"): {"state"}, ("fuse_states", "evidence_in"): {"evidence"},
    ("match_planes", "scan"): {"state"}, ("match_planes", "field"): {"evidence", "fused"},
    ("route_planes", "blocked"): {"fused", "state", "cell ids"}, ("route_planes", "goals"): {"frontier"}, ("route_planes", "cost"): {"fit"},
    ("footprint_planes", "blocked"): {"fused"},
    ("route_headings", "mask"): {"mask"}, ("route_headings", "goals"): {"frontier"}, ("route_headings", "cost"): {"fit"},
    ("track_clusters", "cells"): {"cell ids"}, ("track_clusters", "prev"): {"cell ids"}, ("track_clusters", "tracks_in"): {"tracks"},
    ("track_clusters", "heads_in"): {"heads"},
}
INPUTS = {"fuse_states": ["state", "evidence_in"], "route_planes": ["blocked", "cost", "goals"], "match_planes": ["scan", "field"],
          "footprint_planes": ["blocked"], "route_headings": ["mask", "cost", "goals"], "track_clusters": ["cells", "prev", "tracks_in", "heads_in"]}
PLANE_MUTANTS = [
    "fuse_shift_sign_flipped",            # the evidence is scrolled the other way
    "track_shift_sign_flipped",           # ... and so is the previous id plane
    "plane_shift_last_move_only",         # of several moves between two observations only the last one's shift is passed
    "plane_prior_survives_reset",         # a reset or set_position of a chain's slot does not end the chain
    "track_heads_in_dropped",             # next_id restarts at 0
    "fuse_evidence_of_two_calls_ago",     # the two evidence buffers are not alternated: the prior is the one before the last
    "plane_shift_rows_cols_swapped",      # (s0, s1) passed as (s1, s0)
    "footprint_outside_free_inverted",
    "headings_goal_headings_ignored",     # every heading of a goal cell is a goal state
    "route_cost_unclamped",               # w = max(word, 1), cost_max not applied
    "plane_call_computes_lazy_layers",    # a plane call of n maps computes the lazily kept layers of slots 0 .. n - 1
]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
JUNK = 0x0BADF00D   # between and behind the planes of a foreign input: a word >= 0 (blocked, a goal, occupied) for a kernel that reads too far


# ---------------------------------------------------------------------------------------------------------------- foreign planes

def foreign_plane(spec, i, rows):
    """plane i of a foreign input as a logical int32 [rows, rows] array; `distinct`: how many different planes the rows cycle through"""
    rng = np.random.default_rng([int(spec["seed"]), i % int(spec.get("distinct", 1)), 80])
    kind, shape = spec["kind"], (rows, rows)
    u = rng.random(shape)
    if kind == "signs":      # a state / scan plane: only the sign counts
        zeros = float(spec.get("zeros", 0.35))
        a = np.where(u < 0.45, rng.choice(np.array([-1, -1, -7, I32_MIN]), shape), np.where(u < 0.45 + zeros, 0, rng.choice(np.array([1, 1, 9, I32_MAX]), shape)))
    elif kind == "blocked":  # >= 0 is blocked
        a = np.where(u < 0.8, rng.choice(np.array([-1, -1, -5, I32_MIN]), shape), rng.choice(np.array([0, 1, 17, I32_MAX]), shape))
    elif kind == "goals":    # >= 0 is a goal
        a = np.where(u < 0.985, rng.choice(np.array([-1, -3, I32_MIN]), shape), rng.choice(np.array([0, 0, 4, I32_MAX]), shape))
    elif kind == "cost":     # clamped to [1, cost_max]
        a = rng.integers(-5, 40, shape)
        a = np.where(u < 0.02, I32_MIN, np.where(u > 0.98, I32_MAX, a))
    elif kind == "evidence":  # clamped to [e_min, e_max] / [0, field_max]
        a = rng.integers(-40, 60, shape)
        a = np.where(u < 0.02, I32_MIN, np.where(u > 0.98, I32_MAX, a))
    elif kind == "mask":     # bits 0 .. 31 at random, a quarter of the cells without any
        a = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(np.int32)
        a = np.where(u < 0.25, 0, a)
    elif kind == "tiles":    # a previous id plane that holds an id below `mod` in every cell: whatever lies over it has a predecessor
        side = -(-rows // 6)
        r, c = np.meshgrid(np.arange(rows) // side, np.arange(rows) // side, indexing="ij")
        a = (r * 6 + c + int(rng.integers(0, 7))) % int(spec["mod"])
    elif kind == "cells":    # an id plane: components of a random occupancy; ids beyond max_clusters and words below -1 occur
        a = tracks_ref.label_plane(u < float(spec.get("density", 0.04))).astype(np.int64)
        a = np.where((a < 0) & (rng.random(shape) < 0.05), I32_MIN, a)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a.astype(np.int64).astype(np.int32))


def foreign_tracks(spec, i, M, prev):
    """(records int32 [M, 8], heads int32 [4]) that go with the foreign previous id plane `prev`: what a call without a prior leaves on it,
    with ids that start at a seeded first_id and ages at random"""
    rng = np.random.default_rng([int(spec["seed"]), i % int(spec.get("distinct", 1)), 81])
    rec, heads = tracks_ref.first_records(prev, M, first_id=int(rng.integers(1, 1 << 20)))
    rec[:, 1] = rng.integers(0, 50, M)
    return rec, heads


# ---------------------------------------------------------------------------------------------------------------- the generator

def _plane_pairs(sm, shape, seed):
    """the (predicate, plane kind) pairs the generator of (shape, seed) brings about: every pair in one of the six committed sequences"""
    pairs = [(p, k) for p in sm.PREDICATES for k in PLANE_KINDS]
    pairs = [pairs[i] for i in np.random.default_rng(20261020).permutation(len(pairs))]
    q = 2 * list(sm.SHAPES).index(shape) + int(seed) % sm.SEEDS_PER_SHAPE
    deal = [q2 for q2, share in enumerate((3, 3, 7, 7, 8, 8)) for _ in range(share)]   # (fewest where a reference costs most: the 364-cell shape)
    return [pair for t, pair in enumerate(pairs) if q == deal[t % len(deal)]]


_SIDES = {}


def side_of(sm, shape):
    if shape not in _SIDES:
        from oracle import oracle

        _SIDES[shape] = oracle.OracleMap(sm.SHAPES[shape]["length"], sm.SHAPES[shape]["res"]).rows
    return _SIDES[shape]


class PlaneGen:
    """Inserts ops of PLANE_KINDS -- and the gg_visibility_clouds, gg_cluster_clouds, batches, moves and resets their chains need -- into the
    list `mid`, which stays a subsequence with every dict as it was.  A generator stream of its own; every op it adds carries "g3", its
    ordinal.  In front of the tail it adds nothing that changes a map, so what the older ops meet is what they met.  Sources:
      anchors   behind a batch of the older list on a caller stream: one observation of the body's chain (visibility and clusters of that
                batch's cloud, then the six plane calls), every op on another stream than the one before
      pairs     _plane_pairs, wherever one of slots 0 .. 2 satisfies the predicate: a foreign op of n = slot + 1 maps
      tail      in front of the last checkpoint, with checkpoints of its own: a second chain driven through two moves, a shift beyond a
                side, a set_position, a reset (one script per mutant); the run that goes round the ring; calls of n_slots maps and of
                n_slots + 1"""

    def __init__(self, sm, seed, shape, mid):
        self.sm, self.shape, self.sh, self.seed, self.mid = sm, shape, sm.SHAPES[shape], int(seed), mid
        self.rng = np.random.default_rng([int(seed), list(sm.SHAPES).index(shape), 20261020])
        self.n = self.sh["n_slots"]
        self.rows = side_of(sm, shape)
        self.big = self.rows > 200
        self.out, self.g3 = [], 0
        self.g4 = None   # (the fourth generator stream, tests/seq_late.py, counts here while it adds its ops through this one's push)
        self.pos = [(0.0, 0.0)] * self.n
        self.alive = []
        self.pred = sm.Predicates(self.n)
        self.flags = dict(minimal=False, eager=False, halves=False)
        self.labels_set = False
        self.next_seed = 700000 + 1000 * self.seed
        self.cursor = {}
        self.pending = _plane_pairs(sm, shape, seed)
        self.chains = []
        self.body = None
        self.episodes = 0

    # -- pieces
    def r(self, lo, hi):
        return round(float(self.rng.uniform(lo, hi)), 3)

    def seed_of(self):
        self.next_seed += 1
        return self.next_seed

    def next_of(self, names, attr):
        k = self.cursor.get(attr, 0)
        self.cursor[attr] = k + 1
        return names[k % len(names)]

    def pick(self, values):
        return values[int(self.rng.integers(0, len(values)))]

    def other_stream(self, stream, names=("s1", "s2", "default", "s2", "s1", "ctx", "default")):
        while True:
            s = self.next_of(list(names), "stream " + ",".join(names))
            if s != stream:
                return s

    def push(self, op, mine=True):
        sm, k = self.sm, op["op"]
        if mine:
            op["g3"] = self.g3
            self.g3 += 1
            if self.g4 is not None:
                op["g4"] = self.g4
                self.g4 += 1
        hit = []
        if k == "reset_maps":
            hit = list(range(op["first"], op["first"] + op["n"]))
            for s in hit:
                self.pos[s] = tuple(op["pos"])
        elif k in ("map_reset", "set_position"):
            hit = [op["slot"]]
            self.pos[op["slot"]] = tuple(op["pos"])
        elif k == "move_maps":
            for s, o in zip(op["slots"], op["odoms"]):
                self._moved(s, o)
        elif k == "map_move":
            self._moved(op["slot"], op["odom"])
        elif k == "set_score_labels":
            self.labels_set = True
        elif k == "set_flags":
            self.flags = dict(minimal=op["minimal"], eager=op["eager"], halves=op["halves"])
        elif k == "checkpoint":
            self.alive = []
            for c in self.chains:
                c["written"] = set()
        elif k == "filter_batch" and "labels" in op["outputs"]:
            self.alive.append((len(self.out), op))
        for c in self.chains:   # a reset or set_position of one of its slots ends a chain
            if set(hit) & set(c["of"]):
                if c["fuse"] is not None:
                    c["lost_fuse"], c["fuse"] = c["fuse"], None
                if c["track"] is not None:
                    c["lost_track"], c["track"] = (c["track"], c["clus"]), None
        self.out.append(op)
        self.pred.apply(op)
        if mine and k in PLANE_KINDS and "expect" not in op:
            sl = sm.touched(op, self.n)
            self.pending = [(p, kk) for p, kk in self.pending if not (kk == k and any(self._before[p][s] for s in sl))]

    def _moved(self, s, odom):
        far = max(abs(odom[0] - self.pos[s][0]), abs(odom[1] - self.pos[s][1])) >= 1.5 * self.sh["res"]
        self.pos[s] = tuple(odom)
        for c in self.chains:
            if s in c["of"] and far:
                c["moved_fuse"] = c["moved_track"] = True

    def emit(self, op):
        self._before = {p: list(v) for p, v in self.pred.state.items()}
        self.push(op)
        return len(self.out) - 1

    # -- foreign inputs and parameters
    def foreign(self, kind, distinct=1, **kw):
        if kind == "signs" and self.big:   # (few cells end UNKNOWN: the frontier of fusion_ref walks from every one of them)
            kw["zeros"] = 0.03
        return dict(seed=self.seed_of(), kind=kind, distinct=distinct, **kw)

    def pad(self):
        return self.next_of([0, 3, 0, 29], "pad")

    def fuse_params(self, chained):
        if chained:   # one scan makes a cell free or occupied, so that every observation has a frontier
            return dict(hit=self.pick([3, 4]), miss=self.pick([1, 2]), decay=self.pick([0, 1]), e_min=self.pick([-16, -6]), e_max=self.pick([32, 12]),
                        free_threshold=-1, occ_threshold=3)
        return dict(hit=self.pick([0, 4, 9]), miss=self.pick([0, 1, 3]), decay=self.pick([0, 1, 5]), e_min=self.pick([-16, -50, -2]),
                    e_max=self.pick([32, 7]), free_threshold=self.pick([-1, -2]), occ_threshold=self.pick([1, 4, 7]))

    def want(self, names, must=()):
        got = [k for k in names if k in must or self.rng.random() < 0.7]
        return got

    def mk_fuse(self, n, stream, row_major, state, evidence_in, shifts, chained, must=(), buf=None, chain=None, lost=None):
        pad = self.pad()   # (evidence in and out share plane_stride)
        op = dict(op="fuse_states", n=n, stream=stream, row_major=row_major, state=state, evidence_in=evidence_in, shifts=shifts, pad=pad,
                  in_pad=pad, want=self.want(["fused", "frontier", "counts"], must), buf=buf, chain=chain, **self.fuse_params(chained))
        if lost is not None:
            op["lost"] = lost
        return op

    def mk_route(self, n, stream, row_major, blocked, cost, goals, starts=None):
        conn = self.pick([4, 8])
        return dict(op="route_planes", n=n, stream=stream, row_major=row_major, blocked=blocked, cost=cost, goals=goals, connectivity=conn,
                    straight=self.pick([1, 5]), diagonal=self.pick([7, 2]), cost_max=self.pick([1, 2, 30, 252]), max_cost=self.pick([0, 0, 400]),
                    pad=self.pad(), in_pad=self.pad(), want=self.want(["next", "counts"]), starts=starts, max_path=self.pick([1, 6, 50]))

    def mk_match(self, n, stream, row_major, scan, field, shifts, chain=None):
        K = self.pick([0, 1, 3, 8])
        return dict(op="match_planes", n=n, stream=stream, row_major=row_major, scan=scan, field=field, shifts=shifts, chain=chain,
                    field_max=self.pick([1, 6, 32]), angles=None if K == 0 else [0.0] + [self.r(-0.2, 0.2) for _ in range(K - 1)],
                    window=self.pick([0, 1, 2, 4]), pivots=None if self.rng.random() < 0.5 else [[int(self.rng.integers(0, self.rows)),
                                                                                                  int(self.rng.integers(0, self.rows))] for _ in range(n)],
                    scores=bool(self.rng.random() < 0.7), pad=self.pad(), in_pad=self.pad())

    def mk_footprint(self, n, stream, row_major, blocked, K=None, small=False, outside_free=None):
        K = K or self.pick([1, 4, 8] if not self.big else [1, 4])
        length = self.pick([0, 1, 2])
        half = 0.3 if small else self.pick([0.3, 1.2])
        rect = [footprint_ref.q14(-0.3), footprint_ref.q14(length + 0.3), footprint_ref.q14(-half), footprint_ref.q14(half)]
        need = max(footprint_ref.needed_of(footprint_ref.headings(K), rect), 0)
        want = self.want(["mask", "fit", "counts"], ("mask", "fit") if small else ())
        return dict(op="footprint_planes", n=n, stream=stream, row_major=row_major, blocked=blocked, K=K, rect=rect, radius=max(need, self.pick([need, min(need + 1, 3), 3])),
                    min_fit=int(self.rng.integers(1, K + 1)), outside_free=int(self.rng.integers(0, 2)) if outside_free is None else outside_free,
                    pad=self.pad(), in_pad=self.pad(), want=want or ["counts"])

    def mk_headings(self, n, stream, row_major, mask, cost, goals, K, starts=None):
        return dict(op="route_headings", n=n, stream=stream, row_major=row_major, mask=mask, cost=cost, goals=goals, K=K,
                    goal_headings=self.pick([0xFFFFFFFF, 0xFFFFFFFF, 0x5, 0x1]), step=self.pick([1, 2] if K >= 4 else [1]), unit=10, turn=self.pick([0, 3]),
                    reverse_pct=self.pick([0, 150]), spin=self.pick([0, 4]), cost_max=self.pick([1, 20, 60]), max_cost=self.pick([0, 0, 900]),
                    pad=self.pad(), in_pad=self.pad(), want=self.want(["next", "best", "best_heading", "counts"]), starts=starts, max_len=self.pick([1, 5, 40]))

    def mk_tracks(self, n, stream, row_major, cells, prev, tracks_in, heads_in, shifts, M, gate, buf=None, chain=None, lost=None):
        op = dict(op="track_clusters", n=n, stream=stream, row_major=row_major, cells=cells, prev=prev, tracks_in=tracks_in, heads_in=heads_in,
                  shifts=shifts, M=M, gate=gate, pad=self.pad(), in_pad=self.pad(), cell_track=bool(self.rng.random() < 0.7), buf=buf, chain=chain)
        if lost is not None:
            op["lost"] = lost
        return op

    def seeded_shifts(self, n, far=False):
        """explicit shifts of a foreign op, a different one for neighbouring maps; `far`: one of them beyond the side"""
        # (n > 8: (i % 5, i % 3, i // 15) names i, so no two maps of the call share a shift and a row taken for another shows)
        out = [[(7 * i + 3) % 13 - 6, (5 * i + 1) % 11 - 5] if n <= 8 else [i % 5 - 2, i % 3 - 1 + 3 * (i // 15)] for i in range(n)]
        if far:
            out[0] = [self.rows, -2]
        return dict(values=out)

    def starts(self, n, heading_of=None):
        out = []
        for i in range(n):
            if self.rng.random() < 0.15:
                out.append(None)
            else:
                cell = [int(self.rng.integers(0, self.rows)), int(self.rng.integers(0, self.rows))]
                out.append(cell if heading_of is None else cell + [int(self.rng.integers(0, heading_of))])
        return out

    def mk_foreign(self, kind, n, stream, distinct=None, far=False, sure=False):
        """an op of `kind` on n maps whose every input belongs to no call; `sure`: with a prior, shifts and starts"""
        d = distinct or min(n, 2)
        rm = bool(self.rng.random() < 0.5)
        if kind == "fuse_states":
            prior = self.rng.random() < 0.8 or far or sure
            return self.mk_fuse(n, stream, rm, self.foreign("signs", d), self.foreign("evidence", d) if prior else None,
                                self.seeded_shifts(n, far) if prior and (far or sure or self.rng.random() < 0.85) else None, False)
        if kind == "route_planes":
            return self.mk_route(n, stream, rm, self.foreign("blocked", d) if self.rng.random() < 0.85 else None,
                                 self.foreign("cost", d) if self.rng.random() < 0.7 else None, self.foreign("goals", d),
                                 self.starts(n) if self.rng.random() < 0.7 or sure else None)
        if kind == "match_planes":
            return self.mk_match(n, stream, rm, self.foreign("signs", d), self.foreign("evidence", d), self.seeded_shifts(n, far) if self.rng.random() < 0.8 or far else None)
        if kind == "footprint_planes":
            return self.mk_footprint(n, stream, rm, self.foreign("blocked", d))
        if kind == "route_headings":
            K = self.pick([1, 4, 8] if not self.big else [1, 4])
            return self.mk_headings(n, stream, rm, self.foreign("mask", d), self.foreign("cost", d) if self.rng.random() < 0.6 else None, self.foreign("goals", d), K,
                                    self.starts(n, K) if self.rng.random() < 0.7 else None)
        M = self.pick([1, 3, 64, 1024]) if n <= 2 else self.pick([1, 3, 64])
        prev = self.foreign("tiles" if not far else "cells", d, mod=M)
        shifts = self.seeded_shifts(n, far) if far or self.rng.random() < 0.9 else None
        if shifts is not None and M <= 3 and not far:   # (clusters 0 .. 2 lie in the first lines of the plane: they stay over the previous plane)
            shifts = dict(values=[[abs(a), b] for a, b in shifts["values"]])
        return self.mk_tracks(n, stream, rm, self.foreign("cells", d), prev, dict(foreign=True), dict(foreign=True), shifts, M, int(self.rng.integers(0, 5)))

    # -- chains
    def new_chain(self, of, row_major, M):
        c = dict(id=len(self.chains), of=list(of), row_major=row_major, pad=self.pick([0, 11]), M=M, gate=int(self.rng.integers(0, 5)), fuse=None, buf=0, track=None,
                 clus=None, tbuf=0, written=set(), moved_fuse=False, moved_track=False, lost_fuse=None, lost_track=None, clouds=None, begun=False)
        self.chains.append(c)
        return c

    def cloud_source(self, c, batch):
        """(source, masks) of the chain's cloud calls: rows of `batch` = (index, op), else the chain's own seeded clouds where they were first
        seen (the same scene from scan to scan: what moves is the map)"""
        if batch is not None:
            at, bop = batch
            row0 = bop["slots"].index(c["of"][0])
            src = dict(mode="chained", batch=at, row0=row0, full=True)
            return src, False
        gone = c["clouds"] is not None and any(max(abs(k["cx"] - self.pos[s][0]), abs(k["cy"] - self.pos[s][1])) > 0.25 * self.sh["length"]
                                                for k, s in zip(c["clouds"], c["of"]))   # (the map has left the scene behind: the next one)
        if c["clouds"] is None or gone or c["fuse"] is None and c["track"] is None:
            c["clouds"] = [dict(seed=self.seed_of(), n=int(self.rng.integers(120, min(400, self.sh["stride"]))), kind="scene", cx=self.pos[s][0], cy=self.pos[s][1])
                           for s in c["of"]]
            c["labels"] = dict(seed=self.seed_of())
        stride = min(self.sh["stride"], max(k["n"] for k in c["clouds"]) + 7)
        return dict(mode="foreign", clouds=c["clouds"], labels=c["labels"], fmt=16, tfs=None, stride=stride), False

    def episode(self, c, batch=None, streams=("s1", "s2", "default", "s2", "s1", "ctx", "default"), extra=0):
        """one observation of chain c: the scan's visibility and clusters, then the six plane calls on what they and the chain's last
        observation left; every op on another stream than the one in front of it.  Returns the indices of its ops by kind."""
        n, rm, of = len(c["of"]), c["row_major"], c["of"]
        st = batch[1]["stream"] if batch else None
        source, masks = self.cloud_source(c, batch)
        at = {}

        def nxt():
            nonlocal st
            st = self.other_stream(st, streams)
            return st

        org = [[self.pos[s][0], self.pos[s][1], 0.0] for s in of]
        at["V"] = self.emit(dict(op="visibility_clouds", slots=list(of), source=source, masks=masks, stream=nxt(), min_points=1, min_height=None, max_height=None,
                                 max_cells=0, row_major=rm, pad=c["pad"], origins=org, counts=True))
        at["C"] = self.emit(dict(op="cluster_clouds", slots=list(of), source=source, masks=masks, stream=nxt(), min_points=1, min_height=None, max_height=None,
                                 connectivity=8, row_major=rm, pad=c["pad"], max_clusters=0, point_clusters=False))
        state = dict(op=at["V"], out="state", row0=0)
        cells = dict(op=at["C"], out="cell ids", row0=0)
        prior, lost = c["fuse"], c["lost_fuse"]
        shifts = dict(since=prior, of=list(of)) if prior is not None else None
        if prior is not None:   # the scan against the grid as it stood, then the fusion under the same shift
            at["M"] = self.emit(self.mk_match(n, nxt(), rm, state, dict(op=prior, out=self.pick(["evidence", "fused"]), row0=0), shifts, chain=c["id"]))
        buf = 1 - c["buf"] if prior is not None else c["buf"]
        assert buf not in c["written"]
        fuse = self.mk_fuse(n, nxt(), rm, state, dict(op=prior, out="evidence", row0=0) if prior is not None else None, shifts, True,
                            must=("fused", "frontier"), buf=buf, chain=c["id"],
                            lost=dict(evidence_in=dict(op=lost, out="evidence", row0=0), shifts=dict(since=lost, of=list(of))) if prior is None and lost is not None else None)
        fuse["pad"] = fuse["in_pad"] = c["pad"]   # (the chain's evidence buffers keep one stride)
        at["F"] = self.emit(fuse)
        c["fuse"], c["buf"], c["lost_fuse"], c["moved_fuse"] = at["F"], buf, None, False
        c["written"].add(buf)
        fused, frontier = dict(op=at["F"], out="fused", row0=0), dict(op=at["F"], out="frontier", row0=0)
        if prior is None:       # no grid to match against yet: the scan against its own evidence, no shift
            match = self.mk_match(n, nxt(), rm, state, dict(op=at["F"], out="evidence", row0=0), None, chain=c["id"])
            if lost is not None:
                match["lost"] = {}   # (what the chain lost is no field to match against: the mark alone, for the coverage conditions)
            at["M"] = self.emit(match)
        K = self.pick([4, 8] if not self.big else [4])
        at["P"] = self.emit(self.mk_footprint(n, nxt(), rm, fused, K=K, small=True))
        fit, mask = dict(op=at["P"], out="fit", row0=0), dict(op=at["P"], out="mask", row0=0)
        blocked = self.next_of([fused, state, cells, fused], f"blocked {c['id']}")
        at["R"] = self.emit(self.mk_route(n, nxt(), rm, blocked, fit if self.next_of([True, False, True], "fit") else None, frontier,
                                          self.starts(n) if self.rng.random() < 0.7 else None))
        at["H"] = self.emit(self.mk_headings(n, nxt(), rm, mask, fit if self.rng.random() < 0.4 else None, frontier, K, self.starts(n, K) if self.rng.random() < 0.7 else None))
        tprior, tlost = c["track"], c["lost_track"]
        tbuf = 1 - c["tbuf"] if tprior is not None else c["tbuf"]
        assert ("t", tbuf) not in c["written"]
        if tprior is not None:
            pr = dict(prev=dict(op=c["clus"], out="cell ids", row0=0), tracks_in=dict(op=tprior, out="tracks", row0=0), heads_in=dict(op=tprior, out="heads", row0=0))
        elif tlost is None and not c["begun"]:   # a chain begins on what an earlier session left: planes and records that belong to no call
            pr = dict(prev=self.foreign("tiles", min(n, 2), mod=c["M"]), tracks_in=dict(foreign=True), heads_in=dict(foreign=True))
        else:                                    # ... and after a reset or set_position of one of its slots without a prior
            pr = dict(prev=None, tracks_in=None, heads_in=None)
        c["begun"] = True
        lost = None
        if tprior is None and tlost is not None:
            lost = dict(prev=dict(op=tlost[1], out="cell ids", row0=0), tracks_in=dict(op=tlost[0], out="tracks", row0=0),
                        heads_in=dict(op=tlost[0], out="heads", row0=0), shifts=dict(since=tlost[0], of=list(of)))
        tshifts = dict(since=tprior, of=list(of)) if tprior is not None else self.seeded_shifts(n) if pr["prev"] is not None else None
        at["T"] = self.emit(self.mk_tracks(n, nxt(), rm, cells, pr["prev"], pr["tracks_in"], pr["heads_in"], tshifts,
                                           c["M"], c["gate"], buf=tbuf, chain=c["id"], lost=lost))
        c["track"], c["clus"], c["tbuf"], c["lost_track"], c["moved_track"] = at["T"], at["C"], tbuf, None, False
        c["written"].add(("t", tbuf))
        for j in range(extra):   # (the ring run: every entry is taken once more, by another plane kind than the one before)
            kind = ["match_planes", "footprint_planes", "track_clusters", "match_planes"][j % 4]
            self.emit(self.mk_foreign(kind, 1, nxt()))
        self.episodes += 1
        return at

    # -- where
    def anchors(self, j):
        """behind a batch of the older list on a caller stream: an observation of the body's chain"""
        prev = self.mid[j - 1]
        if prev["op"] != "filter_batch" or not self.alive or self.alive[-1][1] is not prev or self.episodes >= (0 if self.big else 2) or len(prev["slots"]) > 64:
            return
        c = self.body
        if c is None:
            if j < len(self.mid) // 4:
                return
            c = self.body = self.new_chain([prev["slots"][int(self.rng.integers(0, len(prev["slots"])))]], bool(self.seed % 2), self.pick([3, 64]))
        if c["of"][0] not in prev["slots"]:
            return
        fbuf = c["buf"] if c["fuse"] is None else 1 - c["buf"]
        tbuf = c["tbuf"] if c["track"] is None else 1 - c["tbuf"]
        if fbuf in c["written"] or ("t", tbuf) in c["written"]:
            return   # (a chain buffer is written once between two checkpoints)
        if c["fuse"] is not None and not c["moved_fuse"]:
            return   # (nothing moved since its last observation: an all-zero shift)
        self.episode(c, batch=self.alive[-1])

    def pairs(self, j):
        done = 0
        for pred, kind in list(self.pending):
            if done == 1:
                break
            ok = [s for s in range(min(3, self.n)) if self.pred.state[pred][s]]
            if ok:
                self.emit(self.mk_foreign(kind, ok[0] + 1, self.next_of(self.sm.MAP_STREAMS, "pair stream " + kind)))
                done += 1

    def plain(self, j):
        """every kind with no predicate asked for, a few times per sequence, the streams in turn"""
        if self.rng.random() < (0.01 if self.big else 0.035):
            kind = self.next_of(PLANE_KINDS + ["track_clusters"], "plain")
            self.emit(self.mk_foreign(kind, 1 if self.big else int(self.rng.integers(1, min(3, self.n) + 1)), self.next_of(self.sm.MAP_STREAMS, "pair stream " + kind)))

    # -- the tail
    def establish(self, pred, s):
        sm = self.sm
        if pred in ("fresh", "no-confidence"):
            self.push(dict(op="reset_maps", first=s, n=1, odom_z=self.r(-1.9, -1.5), pos=[self.r(-30, 30), self.r(-30, 30)], persistent=False, stream="s1"))
        elif pred == "lazy-owed":
            self.batch([s], "s2")
        elif pred == "own-config":
            self.push(dict(op="set_slot_configs", slots=[s], cfgs=[int(self.rng.integers(1, len(sm.CONFIGS)))]))
        elif pred == "scoring":
            if not self.labels_set:
                self.push(dict(op="set_score_labels", ids=sm.LABEL_LISTS[0]))
            self.push(dict(op="set_scoring", slots=[s], enable=True))
        elif pred == "partly-live":
            self.push(dict(op="set_layer", slot=s, layer="points", fill=dict(seed=self.seed_of(), kind="integer")))

    def batch(self, sl, stream):
        if self.flags["eager"]:
            self.push(dict(op="set_flags", **dict(self.flags, eager=False)))
        lo, hi = self.sh["pts"]
        clouds = [dict(seed=self.seed_of(), n=int(self.rng.integers(lo, hi)), kind="scene", cx=self.pos[t][0], cy=self.pos[t][1]) for t in sl]
        self.push(dict(op="filter_batch", slots=list(sl), clouds=clouds, origins=[[self.pos[t][0], self.pos[t][1], 0.0] for t in sl],
                       base_z=[self.sm.BASE_Z for _ in sl], tfs=None, fmt=16, outputs=["labels", "counts", "masks"], stream=stream))

    def move(self, c, cells, stream, single=False):
        """the chain's maps moved by about `cells` = (rows, cols) cells"""
        res = self.sh["res"]
        if single:
            s = c["of"][0]
            self.push(dict(op="map_move", slot=s, odom=[round(self.pos[s][0] + cells[0] * res, 3), round(self.pos[s][1] + cells[1] * res, 3)],
                           pose=[0.3, 0.2, 1.5, 0.0, 0.0, 0.0, 1.0]))
            return
        self.push(dict(op="move_maps", slots=list(c["of"]), odoms=[[round(self.pos[s][0] + (cells[0] + i) * res, 3), round(self.pos[s][1] + cells[1] * res, 3)]
                                                                     for i, s in enumerate(c["of"])],
                       poses=[[0.3, 0.2, 1.5, 0.0, 0.0, 0.0, 1.0] for _ in c["of"]], stream=stream))

    def tail(self):
        sm = self.sm
        cp = dict(op="checkpoint")
        for pred, kind in list(self.pending):   # what no slot happened to offer
            s = int(self.rng.integers(0, min(3, self.n)))
            self.establish(pred, s)
            self.emit(self.mk_foreign(kind, s + 1, self.next_of(sm.MAP_STREAMS, "pair stream " + kind)))
        self.push(dict(cp))
        # a second chain of two maps (one where max_clusters exceeds what a work-group holds at a time), started behind a batch of its own
        M = [3, 1, 64, 1024, 1024, 64][2 * list(sm.SHAPES).index(self.shape) + self.seed % 2]
        big, odd = self.big, bool(self.seed % 2)
        a = int(self.rng.integers(0, self.n - 1))
        c = self.new_chain([a] if big else [a, a + 1], not odd, M)
        n = len(c["of"])
        two = ("s1", "s2") if not odd else ("default", "s2")
        self.push(dict(op="reset_maps", first=a, n=n, odom_z=self.r(-1.9, -1.5), pos=[self.r(-20, 20), self.r(-20, 20)], persistent=False, stream="s2"))
        self.batch(c["of"], two[0])
        # the run that goes round the ring: a batch, two cloud calls, the six plane kinds and four more, on two caller streams
        self.episode(c, batch=self.alive[-1], streams=two, extra=4)
        # several moves between two observations: the sum of their shifts
        self.move(c, (2, 5), None, single=True)
        self.move(c, (3, -2), "s1")
        self.move(c, (-1, 4), "ctx")
        if not big:   # (in the 364-cell shape one observation is all the references allow); the batch's cloud again: the same scene
            self.episode(c, batch=self.alive[-1])
        self.push(dict(cp))
        if self.shape == "fleet" and not odd:
            # a shift beyond the side: nothing of the prior is left
            far = int(0.6 * self.rows)
            self.move(c, (far, 0), "s2")
            self.move(c, (far, 3), "default")
            self.episode(c)
            self.move(c, (-2, -3), "s1")
            self.move(c, (-3, 1), "s2")
            self.episode(c)          # (overwrites the buffers the observation before it read, on other streams)
            self.push(dict(cp))
        if not big and odd:
            # a set_position of one of its slots ends the chain ...
            s = c["of"][1]
            self.push(dict(op="set_position", slot=s, pos=[round(self.pos[s][0] + 1.0, 3), round(self.pos[s][1] - 0.7, 3)]))
            self.episode(c)
            self.move(c, (4, 4), "s1")
            self.move(c, (1, -6), "s2")
            self.push(dict(cp))
            # ... and so does a reset: of many maps on a stream in the one shape, of one map in the other
            s = c["of"][0]
            if self.shape == "fleet":
                self.push(dict(op="reset_maps", first=s, n=1, odom_z=self.r(-1.9, -1.5), pos=list(self.pos[s]), persistent=True, stream="s1"))
            else:
                self.push(dict(op="map_reset", slot=s, odom_z=self.r(-1.9, -1.5), pos=list(self.pos[s])))
            self.episode(c)
            self.move(c, (-5, 2), "default")
            self.move(c, (2, 2), "s1")
            self.episode(c)
            self.push(dict(cp))
        # foreign calls whose summed shift reaches a side; both values of outside_free and a narrow goal_headings on the chain's planes
        for kind in SHIFTED_KINDS[:2]:
            self.emit(self.mk_foreign(kind, n, self.next_of(sm.MAP_STREAMS, "pair stream " + kind), far=True))
        for _ in range(3 if big else 8):   # (tracks with something to continue: the chains above begin and end without)
            self.emit(self.mk_foreign("track_clusters", int(self.rng.integers(1, 3)), self.next_of(sm.MAP_STREAMS, "pair stream track_clusters")))
        fused, frontier = dict(op=c["fuse"], out="fused", row0=0), dict(op=c["fuse"], out="frontier", row0=0)
        masks = []
        for free in (0, 1) if not big else ():
            masks.append(self.emit(self.mk_footprint(n, self.pick(["s1", "s2"]), c["row_major"], fused, K=4, small=True, outside_free=free)))
        for at, gh in zip(masks, (0x5, 0x2)):
            op = self.mk_headings(n, self.pick(["default", "s1"]), c["row_major"], dict(op=at, out="mask", row0=0), dict(op=at, out="fit", row0=0), frontier, 4,
                                  self.starts(n, 4))
            op["goal_headings"], op["cost_max"] = gh, 2
            self.emit(op)
        if masks:
            op = self.mk_route(n, "s2", c["row_major"], fused, dict(op=masks[0], out="fit", row0=0), frontier, self.starts(n))
            op["cost_max"] = 1
            self.emit(op)
        # the rows of a call to their last: n_slots maps, a few distinct planes, another shift or start for every map; then one map more
        for kind in ("fuse_states", "route_planes"):
            self.emit(self.mk_foreign(kind, self.n, self.next_of(["s1", "s2"], "full"), distinct=1 if big else 3, sure=True))
        kind = ["footprint_planes", "track_clusters", "fuse_states", "route_planes", "match_planes", "route_headings"][2 * list(sm.SHAPES).index(self.shape) + self.seed % 2]
        op = self.mk_foreign(kind, self.n + 1, self.next_of(sm.MAP_STREAMS, "capacity stream"), distinct=1)
        op["expect"] = "GG_ERR_CAPACITY"
        self.emit(op)
        self.emit(self.mk_foreign(kind, 1, op["stream"]))   # (its result shows that the refused call took no ring entry and left no event behind)

    def run(self, late_calls=True):
        n = len(self.mid)
        for j, op in enumerate(self.mid):
            if j == n - 1:
                self.tail()
                if late_calls:   # the fourth generator stream stands behind this one's tail: no index this one's ops name moves
                    from tests import seq_late

                    seq_late.LateGen(self).tail()
            elif j >= 2 and not self.sm._Ins.guarded(self.mid[j - 1]) and not self.sm._Ins.guarded(op):
                self.anchors(j)
                self.pairs(j)
                self.plain(j)
            self.push(op, mine=False)
        return self.out


# ---------------------------------------------------------------------------------------------------------------- what both sides share

def sources_of(op):
    """{input name: source} of a plane op (None for an input left out)"""
    return {name: op[name] for name in INPUTS[op["op"]]}


def is_chained(src):
    return isinstance(src, dict) and "op" in src


def order_of(op):
    return "row" if op["row_major"] else "col"


def summed_shifts(spec, log, mutant=None, kind=None):
    """[n][2] from a shift spec: explicit values, or per slot the sum of the shifts logged for it behind op `since`"""
    if spec is None:
        return None
    if "values" in spec:
        out = [(int(v[0]), int(v[1])) for v in spec["values"]]
    else:
        out = []
        for s in spec["of"]:
            moves = [sh for at, slot, sh in log if slot == s and at > spec["since"]]
            if mutant == "plane_shift_last_move_only":
                moves = moves[-1:]
            out.append((sum(int(m[0]) for m in moves), sum(int(m[1]) for m in moves)))
    if (mutant == "fuse_shift_sign_flipped" and kind == "fuse_states") or (mutant == "track_shift_sign_flipped" and kind == "track_clusters"):
        out = [(-a, -b) for a, b in out]
    if mutant == "plane_shift_rows_cols_swapped":
        out = [(b, a) for a, b in out]
    return out


def spans_of(op):
    return np.array(footprint_ref.rect_spans(footprint_ref.headings(op["K"]), op["rect"], op["radius"]), np.int32)


def moves_of(op):
    return headings_ref.table(op["K"], op["step"], op["unit"], op["turn"], op["reverse_pct"], op["spin"])


def start_cells(op, rows):
    """host `starts` of a route op: linear indices in the op's order, -1 for no start"""
    return [-1 if s is None else route_ref.linear(s[0], s[1], rows, rows, order_of(op)) for s in op["starts"]]


# ---------------------------------------------------------------------------------------------------------------- the model

def _planes_in(cm, src, n, mutant_src=None):
    """the n logical planes of a source, None for a NULL input, "gone" where the op that wrote them is not there (a list with ops deleted)"""
    from tests import seq_model as sm

    if src is None:
        return None
    if is_chained(src):
        rec = cm.outs.get(src["op"])
        if rec is None or src["out"] not in rec or len(rec[src["out"]]) < src["row0"] + n:
            return "gone"
        return rec[src["out"]][src["row0"]: src["row0"] + n]
    d = int(src.get("distinct", 1))
    return [sm._memo(("foreign plane", json.dumps(src, sort_keys=True), i % d, cm.rows), lambda i=i: foreign_plane(src, i, cm.rows)) for i in range(n)]


def _key(op, *skip):
    return json.dumps({k: v for k, v in op.items() if k not in ("stream", "g3", "n", "chain", "buf", "lost", "starts", "shifts", "pad", "in_pad") + skip
                       and k not in INPUTS[op["op"]]}, sort_keys=True)


def model_op(cm, op, m):
    """what the library must return for a plane op, from the references of the six calls applied to the model's own copy of the planes"""
    from tests import seq_model as sm

    kind, n = op["op"], op["n"]
    out = {"fresh maps kept": 1, "lazy maps kept": 1, "nothing else written": 1}
    if "expect" in op:
        return {"error": op["expect"], "nothing written": 1}
    if m == "plane_call_computes_lazy_layers" and any(cm.pred.state["lazy-owed"][s] for s in range(min(n, cm.n))):
        out["lazy maps kept"] = 0
    use = dict(op)
    if m == "plane_prior_survives_reset" and "lost" in op:
        use.update(op["lost"])
    if m == "fuse_evidence_of_two_calls_ago" and kind == "fuse_states" and is_chained(op["evidence_in"]):
        before = cm.outs.get(op["evidence_in"]["op"], {}).get("_op")
        if before is not None and before.get("evidence_in") is not None:
            use["evidence_in"] = before["evidence_in"]
    ins = {name: _planes_in(cm, use[name], n) for name in INPUTS[kind] if name not in ("tracks_in", "heads_in")}
    if any(isinstance(v, str) for v in ins.values()):
        return {"undefined": 1}
    shifts = summed_shifts(use.get("shifts"), cm.shift_log, m, kind)
    order = order_of(op)
    reg = {"_op": op, "_shifts": shifts, "_live": []}   # (_live, per map: something to route to / a cluster with a predecessor: the inertness caps)
    dg = sm._digest

    def put(i, name, v, keep=False):
        out[f"map {i} {name}"] = v
        if keep:
            reg.setdefault(name, []).append(v)

    if kind == "fuse_states":
        p = fusion_ref.params(**{k: op[k] for k in fusion_ref.DEFAULTS})
        for i in range(n):
            ev = ins["evidence_in"][i] if ins["evidence_in"] is not None else None
            sh = shifts[i] if shifts is not None else (0, 0)
            r = sm._memo(("fuse", _key(op, "want"), dg(ins["state"][i]), dg(ev) if ev is not None else b"", sh),
                         lambda: fusion_ref.expected_fusion(ins["state"][i], ev, sh, p))
            put(i, "evidence", r["evidence"], True)
            for name in ("fused", "frontier"):
                if name in op["want"]:
                    put(i, name, r[name], True)
            if "counts" in op["want"]:
                put(i, "counts", r["counts"])
    elif kind == "route_planes":
        p = route_ref.params(connectivity=op["connectivity"], straight=op["straight"], diagonal=op["diagonal"], cost_max=op["cost_max"], max_cost=op["max_cost"])
        if m == "route_cost_unclamped":
            p["cost_max"] = 1000
        starts = start_cells(op, cm.rows) if op["starts"] is not None else None
        for i in range(n):
            b = ins["blocked"][i] if ins["blocked"] is not None else None
            c = ins["cost"][i] if ins["cost"] is not None else None
            r = sm._memo(("route", json.dumps(p, sort_keys=True), order, dg(ins["goals"][i]), dg(b) if b is not None else b"", dg(c) if c is not None else b""),
                         lambda: route_ref.expected_routes(ins["goals"][i], b, c, p, order))
            put(i, "dist", r["dist"])
            reg["_live"].append(bool(r["counts"][1] > r["counts"][0]))
            if "next" in op["want"]:
                put(i, "next", r["next"])
            if "counts" in op["want"]:
                put(i, "counts", r["counts"])
            if starts is not None:
                path = route_ref.path_from(starts[i], r["dist"], r["next"], order)
                put(i, "path length", np.int32(len(path)))
                put(i, "path", np.array(path[: op["max_path"]], np.int32))
    elif kind == "match_planes":
        rot = None if op["angles"] is None else match_ref.rotation_table(op["angles"])
        for i in range(n):
            sh = shifts[i] if shifts is not None else None
            pv = tuple(op["pivots"][i]) if op["pivots"] is not None else None
            r = sm._memo(("match", _key(op, "scores"), dg(ins["scan"][i]), dg(ins["field"][i]), sh, pv),
                         lambda: match_ref.expected_match(ins["scan"][i], ins["field"][i], shift=sh, pivot=pv, rotations=rot, window=op["window"],
                                                          field_max=op["field_max"]))
            put(i, "best", r["best"])
            if op["scores"]:
                put(i, "scores", r["scores"].ravel())
    elif kind == "footprint_planes":
        spans = spans_of(op)
        free = op["outside_free"] if m != "footprint_outside_free_inverted" else 1 - op["outside_free"]
        for i in range(n):
            r = sm._memo(("footprint", _key(op, "want", "outside_free"), free, dg(ins["blocked"][i])),
                         lambda: footprint_ref.expected_footprint(ins["blocked"][i], spans, op["min_fit"], free))
            for name in ("mask", "fit"):
                if name in op["want"]:
                    put(i, name, r[name].view(np.int32) if name == "mask" else r[name], True)
            if "counts" in op["want"]:
                put(i, "counts", r["counts"])
    elif kind == "route_headings":
        moves = moves_of(op)
        gh = op["goal_headings"] if m != "headings_goal_headings_ignored" else headings_ref.ANY
        search = headings_ref.graph_cost_to_go if cm.rows > 200 else headings_ref.cost_to_go
        for i in range(n):
            c = ins["cost"][i] if ins["cost"] is not None else None
            r = sm._memo(("headings", _key(op, "want", "goal_headings", "max_len"), gh, order, dg(ins["mask"][i]), dg(ins["goals"][i]), dg(c) if c is not None else b""),
                         lambda: headings_ref.expected_headings(ins["mask"][i], ins["goals"][i], c, moves, gh, op["cost_max"], op["max_cost"], order, search=search))
            put(i, "dist", r["dist"], True)   # (kept: gg_score_rollouts may be chained to the D volume)
            reg["_live"].append(bool(r["counts"][1] > r["counts"][0]))
            for name in ("next", "best", "best_heading", "counts"):
                if name in op["want"]:
                    put(i, name, r[name])
            if op["starts"] is not None:
                s = op["starts"][i]
                start = (-1, 0) if s is None else (headings_ref.linear(s[0], s[1], cm.rows, cm.rows, order), s[2])
                path = headings_ref.path_from(start, r["dist"], r["next"], moves, order)
                put(i, "path length", np.int32(len(path)))
                put(i, "path", np.array(path[: op["max_len"]], np.int32).reshape(-1, 2))
    else:
        M, g = op["M"], op["gate"]
        prior = ins["prev"] is not None
        for i in range(n):
            tin = hin = None
            if prior:
                if is_chained(use["tracks_in"]):
                    rec = cm.outs.get(use["tracks_in"]["op"])
                    if rec is None or "tracks" not in rec:
                        return {"undefined": 1}
                    tin, hin = rec["tracks"][i], rec["heads"][i]
                else:
                    t, hin = sm._memo(("foreign tracks", json.dumps(use["prev"], sort_keys=True), i % int(use["prev"].get("distinct", 1)), M, cm.rows),
                                      lambda: foreign_tracks(use["prev"], i, M, ins["prev"][i]))
                    tin = np.ascontiguousarray(t).view(tracks_ref.TRACK_DTYPE).reshape(-1)
                if m == "track_heads_in_dropped":
                    hin = np.array([0, hin[1], hin[2], hin[3]], np.int32)
            sh = shifts[i] if shifts is not None else (0, 0)
            key = ("tracks", M, g, dg(ins["cells"][i]), dg(ins["prev"][i]) if prior else b"", dg(tin) if prior else b"", dg(hin) if prior else b"", sh)
            rec, heads, ct = sm._memo(key, lambda: tracks_ref.track_map(ins["cells"][i], ins["prev"][i] if prior else None, tin, hin, sh, M, g))
            put(i, "tracks", np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8))
            put(i, "heads", heads)
            reg.setdefault("tracks", []).append(rec)
            reg.setdefault("heads", []).append(heads)
            reg["_live"].append(bool((rec["prev"] >= 0).any()))
            if op["cell_track"]:
                put(i, "cell track", ct)
    cm.outs[cm.at] = reg
    return out


# ---------------------------------------------------------------------------------------------------------------- the driver

def _source_ptr(d, op, src, n, laid):
    """(address, stride in words) of an input on the device: the earlier op's buffer where it stands, or seeded planes uploaded on the op's
    stream, `in_pad` junk words behind each"""
    cells = d.seg.rows * d.seg.cols
    if src is None:
        return None, 0
    if is_chained(src):
        t, stride, have, row_major = d.dev_outs[src["op"]][src["out"]]
        assert row_major == op["row_major"] and have >= src["row0"] + n, "a chained plane keeps its order"
        return t.data_ptr() + 4 * src["row0"] * stride, stride
    stride = cells + int(op["in_pad"])
    host = np.full((n, stride), JUNK, dtype=np.int32)
    for i in range(n):
        host[i, :cells] = foreign_plane(src, i, d.seg.rows).ravel(order="C" if op["row_major"] else "F")
    laid.append(host)
    return d._upload(host).data_ptr(), stride


def _host_i32(values, keep):
    import ctypes as C

    a = np.ascontiguousarray(np.asarray(values, dtype=np.int32).ravel())
    keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def device_op(d, op):
    """the C call of a plane op on its stream: sentinel-filled destinations with slack words, padded strides; everything is compared at the next
    checkpoint, the words between planes and in the slack included"""
    import ctypes as C

    from groundgrid_amd import _lib, api
    from tests import seq_model as sm

    kind, n, rows = op["op"], op["n"], d.seg.rows
    cells, L, ctx = rows * d.seg.cols, d.seg._L, d.seg._ctx
    order = _lib.GG_PLANES_ROWMAJOR if op["row_major"] else _lib.GG_PLANES_COLMAJOR
    stride = cells + int(op["pad"])
    keep, reg, bufs, reused = [], {}, {}, set()
    shifts = summed_shifts(op.get("shifts"), d.shift_log)

    def dest(name, words, chain_key=None):
        if chain_key is not None:   # a chain's own buffer: filled when it is first used and never again (the call before may still read it)
            if chain_key not in d.chain_bufs:
                d.chain_bufs[chain_key] = d._words(words)
            else:
                reused.add(name)
            bufs[name] = d.chain_bufs[chain_key]
        else:
            bufs[name] = d._words(words)
        return bufs[name].data_ptr()

    with d.on(op["stream"]):
        if kind == "fuse_states":
            x, fn = _lib.GGStateFusion(), L.gg_fuse_states
            x.d_state, x.state_stride = _source_ptr(d, op, op["state"], n, keep)
            x.d_evidence_in, in_stride = _source_ptr(d, op, op["evidence_in"], n, keep)
            assert in_stride in (0, stride), "evidence in and out share plane_stride"
            for k in ("hit", "miss", "decay", "e_min", "e_max", "free_threshold", "occ_threshold"):
                setattr(x, k, op[k])
            x.order, x.plane_stride = order, stride
            x.d_evidence_out = dest("evidence", n * stride, (op["chain"], "evidence", op["buf"]) if op["chain"] is not None else None)
            x.d_fused = dest("fused", n * stride) if "fused" in op["want"] else None
            x.d_frontier = dest("frontier", n * stride) if "frontier" in op["want"] else None
            x.d_counts = dest("counts", n * 4) if "counts" in op["want"] else None
            for name in ("evidence", "fused", "frontier"):
                if name in bufs:
                    reg[name] = (bufs[name], stride, n, op["row_major"])
        elif kind == "route_planes":
            x, fn = _lib.GGPlaneRoutes(), L.gg_route_planes
            x.d_blocked, x.blocked_stride = _source_ptr(d, op, op["blocked"], n, keep)
            x.d_cost, x.cost_stride = _source_ptr(d, op, op["cost"], n, keep)
            x.d_goals, x.goal_stride = _source_ptr(d, op, op["goals"], n, keep)
            for k in ("connectivity", "straight", "diagonal", "cost_max", "max_cost"):
                setattr(x, k, op[k])
            x.order, x.plane_stride = order, stride
            x.d_dist = dest("dist", n * stride)
            x.d_next = dest("next", n * stride) if "next" in op["want"] else None
            x.d_counts = dest("counts", n * 3) if "counts" in op["want"] else None
            if op["starts"] is not None:
                x.starts, x.max_path = _host_i32(start_cells(op, rows), keep), op["max_path"]
                x.d_paths, x.d_path_len = dest("paths", n * op["max_path"]), dest("path_len", n)
        elif kind == "match_planes":
            x, fn = _lib.GGPlaneMatches(), L.gg_match_planes
            x.d_scan, x.scan_stride = _source_ptr(d, op, op["scan"], n, keep)
            x.d_field, x.field_stride = _source_ptr(d, op, op["field"], n, keep)
            x.field_max, x.window, x.order = op["field_max"], op["window"], order
            K = 1 if op["angles"] is None else len(op["angles"])
            if op["angles"] is not None:
                x.rotations, x.n_rotations = _host_i32(api.rotation_table(op["angles"]), keep), K
            if op["pivots"] is not None:
                x.pivots = _host_i32(op["pivots"], keep)
            volume = K * (2 * op["window"] + 1) ** 2
            x.d_best = dest("best", n * 6)
            if op["scores"]:
                x.d_scores, x.score_stride = dest("scores", n * (volume + int(op["pad"]))), volume + int(op["pad"])
        elif kind == "footprint_planes":
            x, fn = _lib.GGPlaneFootprints(), L.gg_footprint_planes
            x.d_blocked, x.blocked_stride = _source_ptr(d, op, op["blocked"], n, keep)
            K, R = op["K"], op["radius"]
            spans = np.zeros((K, 2 * R + 1, 2), np.int32)
            rot, rect = api.rotation_table([2.0 * np.pi * k / K for k in range(K)]), (C.c_int32 * 4)(*op["rect"])
            rc = L.gg_footprint_spans(rot.ctypes.data_as(C.POINTER(C.c_int32)), K, rect, R, spans.ctypes.data_as(C.POINTER(C.c_int32)), None)
            assert rc == _lib.GG_OK, rc
            x.spans = _host_i32(spans, keep)
            x.n_headings, x.radius, x.min_fit, x.outside_free, x.order = K, R, op["min_fit"], op["outside_free"], order
            x.mask_stride = x.fit_stride = stride
            x.d_mask = dest("mask", n * stride) if "mask" in op["want"] else None
            x.d_fit = dest("fit", n * stride) if "fit" in op["want"] else None
            x.d_counts = dest("counts", n * 3) if "counts" in op["want"] else None
            for name in ("mask", "fit"):
                if name in bufs:
                    reg[name] = (bufs[name], stride, n, op["row_major"])
        elif kind == "route_headings":
            x, fn = _lib.GGHeadingRoutes(), L.gg_route_headings
            x.d_mask, x.mask_stride = _source_ptr(d, op, op["mask"], n, keep)
            x.d_cost, x.cost_stride = _source_ptr(d, op, op["cost"], n, keep)
            x.d_goals, x.goal_stride = _source_ptr(d, op, op["goals"], n, keep)
            K = op["K"]
            moves = api.heading_moves(api.rotation_table([2.0 * np.pi * k / K for k in range(K)]), step=op["step"], unit=op["unit"], turn=op["turn"],
                                      reverse_pct=op["reverse_pct"], spin=op["spin"])
            x.goal_headings, x.n_headings, x.moves = op["goal_headings"], K, _host_i32(moves, keep)
            x.cost_max, x.max_cost, x.order = op["cost_max"], op["max_cost"], order
            x.plane_stride = x.next_plane_stride = x.best_stride = x.best_heading_stride = stride
            x.dist_stride = x.next_stride = K * stride + 2
            x.d_dist = dest("dist", n * (K * stride + 2))
            reg["dist"] = (bufs["dist"], K * stride + 2, n, op["row_major"], stride, K)   # (the [n][K] volume: dist_stride, then plane_stride and K)
            x.d_next = dest("next", n * (K * stride + 2)) if "next" in op["want"] else None
            x.d_best = dest("best", n * stride) if "best" in op["want"] else None
            x.d_best_heading = dest("best_heading", n * stride) if "best_heading" in op["want"] else None
            x.d_counts = dest("counts", n * 3) if "counts" in op["want"] else None
            if op["starts"] is not None:
                st = [[-1, 0] if s is None else [headings_ref.linear(s[0], s[1], rows, rows, order_of(op)), s[2]] for s in op["starts"]]
                x.starts, x.max_len, x.path_stride = _host_i32(st, keep), op["max_len"], 2 * op["max_len"] + 1
                x.d_paths, x.d_path_len = dest("paths", n * (2 * op["max_len"] + 1)), dest("path_len", n)
        else:
            x, fn = _lib.GGClusterTracks(), L.gg_track_clusters
            M = op["M"]
            x.d_cells, x.cells_stride = _source_ptr(d, op, op["cells"], n, keep)
            x.d_cells_prev, x.prev_stride = _source_ptr(d, op, op["prev"], n, keep)
            if op["prev"] is not None:
                if is_chained(op["tracks_in"]):
                    x.d_tracks_in = d.dev_outs[op["tracks_in"]["op"]]["tracks"][0].data_ptr()
                    x.d_heads_in = d.dev_outs[op["heads_in"]["op"]]["heads"][0].data_ptr()
                else:
                    made = [foreign_tracks(op["prev"], i, M, foreign_plane(op["prev"], i, rows)) for i in range(n)]
                    x.d_tracks_in = d._upload(np.stack([t for t, _ in made])).data_ptr()
                    x.d_heads_in = d._upload(np.stack([h for _, h in made])).data_ptr()
            x.max_clusters, x.gate, x.order, x.track_stride = M, op["gate"], order, stride
            chain = op["chain"]
            x.d_tracks_out = dest("tracks", n * M * 8, (chain, "tracks", op["buf"]) if chain is not None else None)
            x.d_heads_out = dest("heads", n * 4, (chain, "heads", op["buf"]) if chain is not None else None)
            x.d_cell_track = dest("cell_track", n * stride) if op["cell_track"] else None
            reg["tracks"], reg["heads"] = (bufs["tracks"], M * 8, n, op["row_major"]), (bufs["heads"], 4, n, op["row_major"])
        x.n = n
        if shifts is not None:
            x.shifts = _host_i32(shifts, keep)
        if "expect" in op:   # an argument error: nothing is enqueued, nothing written, no ring entry taken
            if op["stream"] == "ctx":
                d.torch.cuda.current_stream(d.seg.device).synchronize()
            else:
                d.used.add(op["stream"])
            rc = fn(ctx, C.byref(x), d._stream_arg(op["stream"]))
            marks = None
        else:
            marks = d._enqueue(op, lambda st: fn(ctx, C.byref(x), st))
    d.keep.append((bufs, keep))
    d.dev_outs[d.at] = reg

    def collect():
        host = {name: t.cpu().numpy() for name, t in bufs.items()}
        if "expect" in op:
            return {"error": _lib.STATUS.get(rc, rc), "nothing written": int(all(np.all(a.view(np.uint32) == sm.SENTINEL) for a in host.values()))}
        res = d._marks_kept(marks)
        clean = True

        def planes(name, per_map=1, st=stride):
            nonlocal clean
            got, ok = d._planes(host[name], n * per_map, 1, st, op["row_major"])
            clean &= ok
            return got

        def rows_of(name, words, written=None):
            """the n rows of a small buffer, `words` apart; what lies behind them (and behind written[i] words of row i) keeps the sentinel"""
            nonlocal clean
            a = host[name]
            clean &= bool(np.all(a[n * words:].view(np.uint32) == sm.SENTINEL))
            out = []
            for i in range(n):
                row = a[i * words: (i + 1) * words]
                if written is not None:
                    clean &= bool(np.all(row[written[i]:].view(np.uint32) == sm.SENTINEL))
                    row = row[: written[i]]
                out.append(row)
            return out

        if kind == "fuse_states":
            for name in ("evidence", "fused", "frontier"):
                if name in host:
                    for i, p in enumerate(planes(name)):
                        res[f"map {i} {name}"] = p
            if "counts" in host:
                for i, r in enumerate(rows_of("counts", 4)):
                    res[f"map {i} counts"] = r
        elif kind == "route_planes":
            for name in ("dist", "next"):
                if name in host:
                    for i, p in enumerate(planes(name)):
                        res[f"map {i} {name}"] = p
            if "counts" in host:
                for i, r in enumerate(rows_of("counts", 3)):
                    res[f"map {i} counts"] = r
            if "paths" in host:
                lens = [int(v[0]) for v in rows_of("path_len", 1)]
                for i, r in enumerate(rows_of("paths", op["max_path"], [min(max(v, 0), op["max_path"]) for v in lens])):
                    res[f"map {i} path length"], res[f"map {i} path"] = np.int32(lens[i]), r
        elif kind == "match_planes":
            for i, r in enumerate(rows_of("best", 6)):
                res[f"map {i} best"] = r
            if "scores" in host:
                K = 1 if op["angles"] is None else len(op["angles"])
                volume = K * (2 * op["window"] + 1) ** 2
                for i, r in enumerate(rows_of("scores", volume + int(op["pad"]), [volume] * n)):
                    res[f"map {i} scores"] = r
        elif kind == "footprint_planes":
            for name in ("mask", "fit"):
                if name in host:
                    for i, p in enumerate(planes(name)):
                        res[f"map {i} {name}"] = p
            if "counts" in host:
                for i, r in enumerate(rows_of("counts", 3)):
                    res[f"map {i} counts"] = r
        elif kind == "route_headings":
            K = op["K"]
            for name in ("dist", "next"):
                if name in host:
                    a = host[name]
                    clean &= bool(np.all(a[n * (K * stride + 2):].view(np.uint32) == sm.SENTINEL))
                    for i in range(n):
                        body = a[i * (K * stride + 2): (i + 1) * (K * stride + 2)]
                        clean &= bool(np.all(body[K * stride:].view(np.uint32) == sm.SENTINEL))
                        got, ok = d._planes(body[: K * stride], K, 1, stride, op["row_major"])
                        clean &= ok
                        res[f"map {i} {name}"] = np.stack(got)
            for name in ("best", "best_heading"):
                if name in host:
                    for i, p in enumerate(planes(name)):
                        res[f"map {i} {name}"] = p
            if "counts" in host:
                for i, r in enumerate(rows_of("counts", 3)):
                    res[f"map {i} counts"] = r
            if "paths" in host:
                lens = [int(v[0]) for v in rows_of("path_len", 1)]
                for i, r in enumerate(rows_of("paths", 2 * op["max_len"] + 1, [2 * min(max(v, 0), op["max_len"]) for v in lens])):
                    res[f"map {i} path length"], res[f"map {i} path"] = np.int32(lens[i]), r.reshape(-1, 2)
        else:
            M = op["M"]
            heads = rows_of("heads", 4)
            # (records k >= Kc are never written: the sentinel on a buffer's first use, what the call before the last left on a chain's)
            for i, r in enumerate(rows_of("tracks", M * 8, None if "tracks" in reused else [8 * min(max(int(h[1]), 0), M) for h in heads])):
                res[f"map {i} tracks"] = r[: 8 * min(max(int(heads[i][1]), 0), M)].reshape(-1, 8)
                res[f"map {i} heads"] = heads[i]
            if "cell_track" in host:
                for i, p in enumerate(planes("cell_track")):
                    res[f"map {i} cell track"] = p
        res["nothing else written"] = int(clean)
        return res

    return collect
