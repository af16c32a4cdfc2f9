"""Three later calls in the sequence harness of tests/seq_model.py: gg_box_clusters, gg_score_rollouts and gg_clearance_clouds in plane
mode (`clearance_planes` in api.py) as op kinds (LATE_KINDS) -- their generator stream, their part of the model and their part of the
driver.  seq_model.py and seq_planes.py call into this file; nothing here needs a GPU to import.

  box_clusters      reads the positions of the maps it names, on the device, and the d_point_cluster / d_n_clusters buffers of an earlier
                    gg_cluster_clouds: its result depends on map state that a gg_move_maps or gg_reset_maps on another stream changes.
  score_rollouts    carries its host arrays (`starts`, `rotations`) inside the entry of the ring of parameter blocks, and reads up to four
                    planes that up to four earlier calls wrote: the mask and the fit of gg_footprint_planes, the D volume of
                    gg_route_headings and a squared-distance plane.
  clearance_planes  the producer of that squared-distance plane from an occupancy plane the caller holds.

  input     as in tests/seq_planes.py: CHAINED, {"op": index, "out": name, "row0": r} -- the device buffer the op at that index wrote, as
            it stands (its stride, padding and order; for the D volume its plane_stride and dist_stride too) -- or FOREIGN, seeded words
            that belong to no call.  A box call's points are those of the cluster call it is chained to: that call's batch, or that
            call's own foreign clouds where they lie on the device.
  where     The fourth generator stream stands BEHIND the third one's tail, in front of the last checkpoint: every op of the third stream
            names other ops by their index in the list, and nothing in front of them may move.  Its ops carry "g4", their ordinal (and
            "g3", which goes on counting the ops inserted behind the second stream's list).
  buffers   two squared-distance buffers outlive checkpoints ("buf": 0 / 1): a call overwrites one that a gg_score_rollouts on another
            stream read since the last checkpoint.  Each is written at most once between two checkpoints, so that every output can be
            compared there.

What the model relies on across streams is the header's ORDER OF THE MANY-MAP CALLS ACROSS STREAMS, as in seq_planes.py: the driver puts
its fills and uploads on the stream of the op they belong to, downloads nothing before the checkpoint, and compares every word there.
"""
from __future__ import annotations

import json

import numpy as np

from tests import box_ref, clearance_ref, footprint_ref, headings_ref, rollouts_ref
from tests import seq_planes as sp

LATE_KINDS = ["box_clusters", "score_rollouts", "clearance_planes"]
ROW_KINDS = ("score_rollouts", "clearance_planes")   # map i of the call is row i of its buffers; a box call names slots
# the chains the header names: (kind, input) -> the outputs it is chained to somewhere in the committed sequences
CHAIN_TABLE = {
    ("box_clusters", "point_cluster"): {"point ids"}, ("box_clusters", "n_clusters"): {"clusters"},
    ("clearance_planes", "seeds"): {"fused", "cell ids", "state"},
    ("score_rollouts", "mask"): {"mask"}, ("score_rollouts", "cost"): {"fit"}, ("score_rollouts", "dist"): {"dist"},
    ("score_rollouts", "clear"): {"dist2"},
}
CLEAR_PRODUCERS = {"clearance_planes", "clearance_clouds"}   # a chained `clear` occurs behind either
INPUTS = {"box_clusters": ["point_cluster", "n_clusters"], "score_rollouts": ["mask", "cost", "dist", "clear"], "clearance_planes": ["seeds"]}
LATE_MUTANTS = [
    "box_position_of_before_the_move",        # the boxes are computed under the position from before the last move
    "box_cluster_count_unclamped",            # M_i = max(d_n_clusters[i], 0): records beyond max_clusters
    "box_ids_of_the_previous_cluster_call",   # the ids of the cluster call before the one named
    "rollouts_start_heading_ignored",         # the relative frame rotates by heading 0
    "rollouts_starts_of_the_previous_call",   # the ring-entry slip: the starts of the gg_score_rollouts before this one
    "rollouts_table_of_map_0_for_all",        # per-map tables: every map scores map 0's
    "rollouts_dist_of_two_calls_ago",         # the D volume of the gg_route_headings before the one before the one named
    "rollouts_cost_unclamped",                # w = max(word, 1), cost_max not applied
    "clearance_planes_sign_inverted",         # a seed is a word < 0
]
BOX_M, BOX_K = [1, 3, 64, 256], [1, 5, 32]
ROLLOUT_P = [1, 63, 65]          # in every shape; 1025 once per shape
MAX_T, MAX_PT = 12, 4096
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NONE = rollouts_ref.NONE


# ---------------------------------------------------------------------------------------------------------------- seeded inputs

def foreign_ids(spec, i, n_points, M):
    """the d_point_cluster words of cloud i that belong to no cluster call: mostly ids of [0, M), and words below -1, INT32_MIN and ids >= M"""
    rng = np.random.default_rng([int(spec["seed"]), i, 83])
    ids = rng.integers(0, M, n_points).astype(np.int64)
    odd = rng.choice(np.array([-1, -2, -7, I32_MIN, M, M + 5, I32_MAX], np.int64), n_points)
    return np.where(rng.random(n_points) < 0.12, odd, ids).astype(np.int32)


def foreign_count(spec, i, M):
    """the d_n_clusters word of cloud i: M, words above it, below it, and negative ones"""
    return int([M, M + 7, max(1, M // 2), -3, M, I32_MAX, max(1, M - 1)][(int(spec["seed"]) + i) % 7])


def box_angles(K):
    """K candidate headings of a rectangle: angles in [0, pi / 2)"""
    return [0.5 * np.pi * k / K for k in range(K)]


def make_table(spec, i, K, side):
    """the table of map i (of every map when it is shared), int32 [T, P, 4] of (da, db, dk, s): rollouts that move a few sixteenths to a
    few cells per step, a tenth of them fast enough to leave the map; every seventh ends early (s == 0 or negative), every eleventh is
    empty (s <= 0 at t = 0, "stay"); dk runs negative and beyond K; s beyond 32767 here and there.  Absolute tables wander from the middle
    of the map.  A table of one rollout holds one step within a cell of where it starts."""
    P, T = int(spec["P"]), int(spec["T"])
    rng = np.random.default_rng([int(spec["seed"]), i if spec["pad"] else 0, 82])
    v = rng.integers(-40, 41, (P, 2)) * (P > 1)
    if P > 1:
        fast = rng.random(P) < 0.1
        v = np.where(fast[:, None], v * max(1, (16 * side) // (40 * T)), v)
    t = np.arange(1, T + 1).reshape(T, 1)
    jitter = rng.integers(-6, 7, (T, P, 2))
    da, db = v[None, :, 0] * t + jitter[..., 0], v[None, :, 1] * t + jitter[..., 1]
    if not spec["relative"]:
        da, db = da + 16 * (side // 2) + 8, db + 16 * (side // 2) + 8
    dk = rng.integers(-3 * K - 1, 3 * K + 2, (T, P))
    s = rng.integers(1, 40, (T, P))
    s[rng.random((T, P)) < 0.01] = 40000
    p = np.arange(P)
    if P > 1:
        cut = rng.integers(0, T, P)
        ends = (t - 1 == cut[None, :]) & (p % 7 == 3)[None, :]
        s = np.where(ends, np.where(p % 2 == 0, 0, -7)[None, :], s)
        s[0, :] = np.where(p % 11 == 5, 0, s[0, :])
    else:
        s[1:, :] = 0
    return np.stack([da, db, dk, s], axis=-1).astype(np.int32)


def dist_volume(src, i, K, rows):
    """the K planes of map i of a foreign D volume: words of either sign, GG_ROUTE_NONE (INT32_MAX) and INT32_MIN among them"""
    d = max(1, int(src.get("distinct", K)) // K)
    return np.stack([sp.foreign_plane(src, (i % d) * K + k, rows) for k in range(K)])


def start_words(op):
    """host `starts` [n][3]: (-1, 0, 0) for a map without a start"""
    return [[-1, 0, 0] if s is None else [int(v) for v in s] for s in op["starts"]]


def chained_inputs(op):
    return {name: op[name] for name in INPUTS[op["op"]] if sp.is_chained(op[name])}


def _late_pairs(sm, shape, seed):
    """the (predicate, late kind) pairs the generator of (shape, seed) brings about: every pair in one of the six committed sequences"""
    pairs = [(p, k) for p in sm.PREDICATES for k in LATE_KINDS]
    pairs = [pairs[i] for i in np.random.default_rng(20261021).permutation(len(pairs))]
    q = 2 * list(sm.SHAPES).index(shape) + int(seed) % sm.SEEDS_PER_SHAPE
    return [pair for t, pair in enumerate(pairs) if t % (len(sm.SHAPES) * sm.SEEDS_PER_SHAPE) == q]


# ---------------------------------------------------------------------------------------------------------------- the generator

class LateGen:
    """The fourth generator stream: ops of LATE_KINDS -- and the cluster, footprint, heading, fusion, clearance and visibility calls, the
    batches, moves and resets their chains need -- behind the tail of the third stream `g` (seq_planes.PlaneGen), through that one's push,
    so that positions, predicates and alive batches go on being tracked in one place.  Sections, a checkpoint behind each:
      pairs     _late_pairs: the predicate brought about on one of slots 0 .. 2, then a foreign op that names the slot
      first     a squared-distance plane into a buffer that outlives the checkpoint
      ring      one run on two caller streams: a batch, its clusters, moves, a footprint and a heading call, two clearance calls, two box
                calls and five rollout calls with pairwise different starts, no two of them side by side; every entry of the ring is taken by a late kind and later by
                another kind; the rollouts read what calls on the other stream wrote; the second clearance call overwrites the buffer of
                `first`, which a rollout call on the other stream read
      chains    the rest of CHAIN_TABLE; a reset between a cluster call and the box call that reads it; a second cluster call in front of
                the one a box call names; foreign ids and counts; both point formats, transforms, a slot list and first_slot
      rows      once per shape and kind a call of n_slots maps, one map more refused, and a call behind it on the same stream"""

    def __init__(self, g):
        self.g, self.sm = g, g.sm
        self.q = 2 * list(g.sm.SHAPES).index(g.shape) + g.seed % 2
        self.rng = np.random.default_rng([g.seed, list(g.sm.SHAPES).index(g.shape), 20261021])
        self.rows, self.n, self.big = g.rows, g.n, g.big
        self.cursor = {}
        last = g.chains[-1]   # (the third stream's last chain as its tail left it: a reset of this stream's ends it)
        assert last["fuse"] is not None and "fused" in g.out[last["fuse"]]["want"]
        self.fused = (last["fuse"], len(last["of"]), last["row_major"])
        g.g4 = 0

    # -- pieces
    def turn(self, values, attr):
        """the values in turn, the six sequences starting at different ones"""
        k = self.cursor.get(attr, self.q)
        self.cursor[attr] = k + 1
        return values[k % len(values)]

    def pick(self, values):
        return values[int(self.rng.integers(0, len(values)))]

    def emit(self, op):
        return self.g.emit(op)

    def checkpoint(self):
        self.g.push(dict(op="checkpoint"))

    def foreign(self, kind, distinct=1, **kw):
        return self.g.foreign(kind, distinct, **kw)

    def cloud_source(self, slots, tf=None, fmt=None):
        """foreign clouds for `slots`, a scene around each map's position; with transforms the clouds lie round the origin"""
        g = self.g
        tf = bool(self.rng.random() < 0.4) if tf is None else tf
        clouds, tfs = [], []
        for s in slots:
            cx, cy = (0.0, 0.0) if tf else g.pos[s]
            clouds.append(dict(seed=g.seed_of(), n=int(self.rng.integers(30, min(200, g.sh["stride"]))), kind="scene", cx=cx, cy=cy))
            th = float(self.rng.uniform(-0.6, 0.6))
            tfs.append([g.pos[s][0], g.pos[s][1], 0.0, 0.0, 0.0, float(np.sin(th / 2)), float(np.cos(th / 2))])
        stride = min(g.sh["stride"], max(c["n"] for c in clouds) + int(self.pick([0, 1, 7])))
        return dict(mode="foreign", clouds=clouds, labels=dict(seed=g.seed_of()), fmt=fmt or int(self.pick([16, 32])), tfs=tfs if tf else None, stride=stride)

    def batch_source(self, slots):
        at, bop = self.g.alive[-1]
        assert bop["slots"][: len(slots)] == list(slots)
        return dict(mode="chained", batch=at, row0=0, full=True)

    def mk_clusters(self, slots, source, stream, rm, min_points=1, connectivity=8):
        return dict(op="cluster_clouds", slots=list(slots), source=source, masks=False, stream=stream, min_points=min_points, min_height=None, max_height=None,
                    connectivity=connectivity, row_major=rm, pad=self.g.pad(), max_clusters=0, point_clusters=True)

    def mk_box(self, stream, cluster=None, slots=None, source=None, n=None):
        """a box call: chained to the cluster call at index `cluster` of the list (that call's slots and points), else foreign ids and
        counts on `source`"""
        g = self.g
        if cluster is not None:
            made = g.out[cluster]
            slots, source = list(made["slots"]), made["source"]
            ids, counts = dict(op=cluster, out="point ids", row0=0), dict(op=cluster, out="clusters", row0=0)
        else:
            ids, counts = dict(seed=g.seed_of()), dict(seed=g.seed_of())
        run = all(b == a + 1 for a, b in zip(slots, slots[1:]))
        return dict(op="box_clusters", n=len(slots), slots=list(slots), slot_list=bool(not run or self.turn([True, False], "slot list")), source=source,
                    point_cluster=ids, n_clusters=counts, K=self.turn(BOX_K, "box K"), criterion=self.turn(["edge", "area", "area", "edge"], "criterion"),
                    M=self.turn(BOX_M + [64], "box M"), costs=self.turn([True, False, True], "costs"), stream=stream)

    def mk_clearance(self, n, stream, rm, seeds, buf=None, pad=None, nearest=None):
        nearest = (self.shape_small() and bool(self.rng.random() < 0.7)) if nearest is None else nearest
        return dict(op="clearance_planes", n=n, stream=stream, row_major=rm, seeds=seeds, max_cells=self.pick([0, 0, 5, 20]), nearest=nearest,
                    distance=bool(self.rng.random() < 0.6), count=bool(self.rng.random() < 0.7), pad=self.g.pad() if pad is None else pad,
                    in_pad=self.g.pad(), buf=buf)

    def shape_small(self):
        return not self.big

    def table(self, P, T, relative, per_map):
        assert P * T <= MAX_PT and T <= MAX_T
        return dict(seed=self.g.seed_of(), P=P, T=T, relative=relative, pad=self.turn([1, 3, 5], "table pad") if per_map else 0)

    def random_start(self, K):
        lo, hi = self.rows // 2 - min(self.rows // 4, 12), self.rows // 2 + min(self.rows // 4, 12)
        sub = [0, 8, 15]
        return [16 * int(self.rng.integers(lo, hi)) + self.pick(sub), 16 * int(self.rng.integers(lo, hi)) + self.pick(sub), int(self.rng.integers(0, K))]

    def goal_start(self, foot, head, i):
        """a start of map i on a goal state of the heading call at index `head` (D == 0 there: the rollout that stays is scored), whose
        mask the footprint call at `foot` wrote; both calls read seeded planes, so their references can be asked here"""
        g, sm = self.g, self.sm
        P, H = g.out[foot], g.out[head]
        blocked = sm._memo(("foreign plane", json.dumps(P["blocked"], sort_keys=True), i % int(P["blocked"].get("distinct", 1)), self.rows),
                           lambda: sp.foreign_plane(P["blocked"], i, self.rows))
        r = sm._memo(("footprint", sp._key(P, "want", "outside_free"), P["outside_free"], sm._digest(blocked)),
                     lambda: footprint_ref.expected_footprint(blocked, sp.spans_of(P), P["min_fit"], P["outside_free"]))
        goals = sp.foreign_plane(H["goals"], i, self.rows)
        states = np.argwhere(headings_ref.goal_states(r["mask"], goals, H["K"], H["goal_headings"]))
        if not len(states):
            return self.random_start(H["K"])
        k, row, col = (int(v) for v in states[int(self.rng.integers(0, len(states)))])
        return [16 * row + self.pick([0, 8, 15]), 16 * col + self.pick([0, 8, 15]), k]

    def mk_rollouts(self, n, stream, rm, K, mask, cost=None, dist=None, clear=None, starts=None, P=None, T=None, relative=None, per_map=None, best=None):
        P = self.turn([63, 65, 17, 200, 9], "P") if P is None else P   # (a single rollout: once per shape, in the run that goes round the ring)
        T = (int(self.rng.integers(1, MAX_T + 1)) if P * MAX_T <= MAX_PT else max(1, MAX_PT // P)) if T is None else T
        T = min(T, MAX_PT // P, MAX_T)
        relative = self.turn([True, False, True], "frame") if relative is None else relative
        per_map = self.turn([False, True], "per map") if per_map is None else per_map
        if starts is None:
            starts = [self.random_start(K) for _ in range(n)]
        return dict(op="score_rollouts", n=n, stream=stream, row_major=rm, mask=mask, cost=cost, dist=dist, clear=clear, K=K, starts=starts, relative=relative,
                    table=self.table(P, T, relative, per_map), cost_max=self.pick([1, 20, 252]), reach=self.turn([0, 1, 63, 0], "reach"),
                    best=self.turn([True, True, False], "best") if best is None else best, pad=self.turn([0, 3, 0, 5], "record pad"), in_pad=self.g.pad())

    def foreign_rollouts(self, n, stream, K=None, rm=None, clear=False, **kw):
        """a rollout call whose planes belong to no call (`clear`: the one that does, chained)"""
        K = K or self.pick([1, 4] if self.big else [1, 4, 8])
        d = min(n, 2)
        opt = lambda kind, dd=d: self.foreign(kind, dd) if self.rng.random() < 0.6 else None   # noqa: E731
        starts = [self.random_start(K) for _ in range(n)]
        if n >= 2 and self.turn([True, False], "no start"):
            starts[int(self.rng.integers(0, n))] = None
        dist = self.foreign("cost", d * K) if self.rng.random() < 0.6 else None   # (words below 0, INT32_MIN and GG_ROUTE_NONE among them)
        return self.mk_rollouts(n, stream, bool(self.rng.random() < 0.5) if rm is None else rm, K, self.foreign("mask", d), opt("cost"), dist,
                                opt("evidence") if clear is False else clear, starts=starts, **kw)

    def foreign_op(self, kind, slot, stream):
        """an op of `kind` that names `slot`, every input foreign"""
        if kind == "box_clusters":
            others = [s for s in range(self.n) if s != slot]
            slots = [slot] + [others[int(i)] for i in self.rng.permutation(len(others))[: int(self.rng.integers(0, 3))]]
            if self.turn([False, True], "pair run"):
                slots = [slot, slot + 1] if slot + 1 < self.n else [slot - 1, slot]
            return self.mk_box(stream, slots=slots, source=self.cloud_source(slots))
        if kind == "score_rollouts":
            return self.foreign_rollouts(slot + 1, stream)
        return self.mk_clearance(slot + 1, stream, bool(self.rng.random() < 0.5), self.foreign(self.pick(["goals", "cells"]), min(slot + 1, 2)))

    # -- the sections
    def pairs(self):
        sm = self.sm
        for j, (pred, kind) in enumerate(_late_pairs(sm, self.g.shape, self.g.seed)):
            s = int(self.rng.integers(0, min(3, self.n)))
            self.g.establish(pred, s)
            self.emit(self.foreign_op(kind, s, sm.MAP_STREAMS[(self.q + j + LATE_KINDS.index(kind)) % 4]))
        self.checkpoint()

    def ring(self):
        g = self.g
        odd = bool(g.seed % 2)
        a, b = ("s1", "s2") if odd else ("default", "s2")
        rm = not odd
        nP = 1 if self.big else 2            # maps of the calls whose references search (footprint, headings)
        K = 4 if self.big else self.pick([4, 8])
        s0 = int(self.rng.integers(0, self.n - 1))
        of = [s0, s0 + 1]
        c = dict(of=of)
        pad = self.pick([0, 11])
        # `first`: a squared-distance plane left in a buffer of its own, compared at the checkpoint behind it
        L0 = self.emit(self.mk_clearance(nP, b, rm, self.foreign("goals", nP), buf=0, pad=pad))
        g.push(dict(op="reset_maps", first=s0, n=2, odom_z=g.r(-1.9, -1.5), pos=[g.r(-20, 20), g.r(-20, 20)], persistent=False, stream="s2"))
        self.checkpoint()
        # the run
        g.batch(of, a)
        # (ring entries in turn: clusters, R1, footprint, box | R2, headings, clearance, R3 | clearance, R4, box, R5 -- no two rollout calls
        # side by side, and every entry is taken by a late kind and later by another kind)
        C1 = self.emit(self.mk_clusters(of, self.batch_source(of), b, rm))
        self.emit(self.foreign_rollouts(nP, a, K=K, rm=rm, clear=dict(op=L0, out="dist2", row0=0)))   # (reads what `first` left; a clearance call of the run overwrites it)
        P = self.emit(g.mk_footprint(nP, b, rm, self.foreign("blocked", nP), K=K, small=True))
        mask, fit = dict(op=P, out="mask", row0=0), dict(op=P, out="fit", row0=0)
        g.move(c, (3, -2), a)
        self.emit(self.mk_box(b, cluster=C1))                                                      # a move on the other stream in front of it ...
        g.move(c, (-1, 4), a)                                                                      # ... and one behind it
        self.emit(self.mk_rollouts(nP, a, rm, K, mask, cost=fit, relative=True, per_map=nP > 1, P=65))
        H = self.emit(g.mk_headings(nP, b, rm, mask, fit if self.rng.random() < 0.5 else None, self.foreign("goals", nP), K))
        g.out[-1]["max_cost"] = 0
        dist = dict(op=H, out="dist", row0=0)
        L1 = self.emit(self.mk_clearance(nP, a, rm, dict(op=C1, out="cell ids", row0=0), buf=1, pad=pad, nearest=False))
        seen = []

        def starts():
            for _ in range(50):
                st = [self.goal_start(P, H, i) for i in range(nP)]
                if st not in seen:
                    break
            seen.append(st)
            return st

        clear1 = dict(op=L1, out="dist2", row0=0)
        self.emit(self.mk_rollouts(nP, b, rm, K, mask, dist=dist, clear=clear1, starts=starts(), P=63, best=True))
        self.emit(self.mk_clearance(nP, b, rm, self.foreign("cells", nP), buf=0, pad=pad))         # overwrites what the first rollout call of the run read on `a`
        big_p = not odd   # (the 1024-thread stride loop: once per shape)
        self.emit(self.mk_rollouts(nP, a, rm, K, mask, cost=fit, dist=dist, clear=clear1, starts=starts(), P=1025 if big_p else 1, T=3 if big_p else None, per_map=False,
                                   relative=True))
        self.emit(self.mk_box(a, cluster=C1))
        self.emit(self.mk_rollouts(nP, b, rm, K, self.foreign("mask", nP), dist=dist, starts=starts(), relative=False, best=False))
        self.checkpoint()
        return of, (a, b)

    def chains(self, of, two):
        g = self.g
        a, b = two
        rm = bool(self.rng.random() < 0.5)
        g.batch(of, b)
        src = self.batch_source(of)
        org = [[g.pos[s][0], g.pos[s][1], 0.0] for s in of]
        V = self.emit(dict(op="visibility_clouds", slots=list(of), source=src, masks=False, stream=a, min_points=1, min_height=None, max_height=None,
                           max_cells=0, row_major=rm, pad=g.pad(), origins=org, counts=False))
        # (most cells of a state plane and of a fused plane are seeds: the brute-force reference of `nearest` is for the sparse seeded planes)
        self.emit(self.mk_clearance(len(of), b, rm, dict(op=V, out="state", row0=0), nearest=False))
        at, rows_made, order = self.fused
        self.emit(self.mk_clearance(rows_made, self.pick(["ctx", "default"]), order, dict(op=at, out="fused", row0=0), nearest=False))
        CC = self.emit(dict(op="clearance_clouds", slots=list(of), source=src, masks=True, stream=a, min_points=1, min_height=None, max_height=None, max_cells=0,
                            row_major=rm, pad=g.pad(), nearest=False, distance=False))
        K = self.pick([1, 4])
        self.emit(self.foreign_rollouts(len(of), b, K=K, rm=rm, clear=dict(op=CC, out="dist2", row0=0)))
        # two cluster calls on the same clouds, the box call reads the second; then a reset between the clusters and the boxes
        # (the first keeps clusters of two points and more only, so that its ids differ; the second keeps every obstacle point: the cap on inert box calls)
        self.emit(self.mk_clusters(of, src, a, rm, min_points=2, connectivity=4))
        C2 = self.emit(self.mk_clusters(of, src, "ctx", rm, min_points=1, connectivity=8))
        self.emit(self.mk_box(b, cluster=C2))
        g.push(dict(op="reset_maps", first=of[0], n=1, odom_z=g.r(-1.9, -1.5), pos=[round(g.pos[of[0]][0] + 1.3, 3), round(g.pos[of[0]][1] - 0.9, 3)],
                    persistent=bool(g.seed % 2), stream=a))
        self.emit(self.mk_box(b, cluster=C2))
        g.push(dict(op="reset_maps", first=of[1], n=1, odom_z=g.r(-1.9, -1.5), pos=[round(g.pos[of[1]][0] - 0.7, 3), round(g.pos[of[1]][1] + 2.1, 3)],
                    persistent=False, stream=a))
        # clouds that belong to no batch: both point formats, with and without transforms; ids and counts that belong to no cluster call
        others = [s for s in range(self.n) if s not in of][:2] or of[:1]
        CF = self.emit(self.mk_clusters(others, self.cloud_source(others, tf=bool(g.seed % 2), fmt=32 if g.seed % 2 else 16), b, rm))
        g.move(dict(of=others), (2, 3), b)
        self.emit(self.mk_box(self.pick(["ctx", "default"]), cluster=CF))
        slots = list(range(of[0], min(of[0] + 3, self.n)))
        self.emit(self.mk_box("ctx", slots=slots, source=self.cloud_source(slots, tf=not g.seed % 2, fmt=16 if g.seed % 2 else 32)))
        for _ in range(2):
            self.emit(self.foreign_rollouts(int(self.rng.integers(2, 4)), self.turn(self.sm.MAP_STREAMS, "plain stream")))
        self.checkpoint()

    def full_rows(self):
        """the rows of a call to their last, then one map more; which kinds: dealt over the two seeds of a shape"""
        g, n = self.g, self.n
        kinds = ["box_clusters", "score_rollouts"] if g.seed % 2 == 0 else ["clearance_planes"]
        for kind in kinds:
            stream = self.turn(["s1", "s2", "default"], "capacity stream")
            for count, expect in ((n, None), (n + 1, "GG_ERR_CAPACITY"), (1, None)):
                if kind == "box_clusters":
                    slots = list(range(min(count, n)))
                    src = self.cloud_source(slots)
                    for c in src["clouds"]:
                        c["n"] = min(c["n"], 40)
                    src["stride"] = 48
                    if count > n:   # (the cloud of the map that is not there)
                        slots.append(n)
                        src["clouds"].append(dict(src["clouds"][-1]))
                        if src["tfs"]:
                            src["tfs"].append(list(src["tfs"][-1]))
                    op = self.mk_box(stream, slots=slots, source=src)
                    op["slot_list"] = bool(count == 1)
                elif kind == "score_rollouts":
                    op = self.foreign_rollouts(count, stream, K=self.pick([1, 4]), P=self.pick([7, 16]), T=2)
                    op["starts"] = [None if i % 5 == 3 else [16 * (self.rows // 2 - 2 + i % 5) + i % 16, 16 * (self.rows // 2 - 1 + i % 3) + (3 * i) % 16, i % op["K"]]
                                    for i in range(count)]
                else:
                    op = self.mk_clearance(count, stream, bool(g.seed % 2), self.foreign("goals", 3), nearest=False)
                if expect:
                    op["expect"] = expect
                self.emit(op)

    def tail(self):
        self.pairs()
        of, two = self.ring()
        self.chains(of, two)
        self.full_rows()


# ---------------------------------------------------------------------------------------------------------------- the model

def _base():
    return {"fresh maps kept": 1, "lazy maps kept": 1, "nothing else written": 1, "inputs as they were": 1}


def _key(op, *skip):
    return json.dumps({k: v for k, v in op.items() if k not in ("stream", "g3", "g4", "n", "buf", "pad", "in_pad", "starts", "slots", "slot_list", "source", "best") + skip
                       and k not in INPUTS[op["op"]]}, sort_keys=True)


def _box_model(cm, op, m, out, reg):
    from tests import seq_model as sm

    n, M, K = op["n"], op["M"], op["K"]
    clouds = cm._labelled(dict(slots=op["slots"], source=op["source"]))
    if clouds is None:
        return None
    ids_src, cnt_src = op["point_cluster"], op["n_clusters"]
    ids = counts = None
    if sp.is_chained(ids_src):
        at = ids_src["op"]
        if m == "box_ids_of_the_previous_cluster_call":   # (of the cluster calls that left as many rows of ids)
            before = [j for j in sorted(cm.outs) if j < at and len(cm.outs[j].get("point ids", ())) >= n]
            at = before[-1] if before else at
        rec, rec_n = cm.outs.get(at), cm.outs.get(cnt_src["op"])
        if rec is None or rec_n is None or len(rec.get("point ids", ())) < n or len(rec_n.get("clusters", ())) < n:
            return None
        ids, counts = rec["point ids"], [int(v) for v in rec_n["clusters"]]
    rot = box_ref.rotation_table(box_angles(K))
    criterion = box_ref.EDGE if op["criterion"] == "edge" else box_ref.AREA
    for i, (s, cloud, _) in enumerate(clouds):
        ref, sl = cm.slots[s].ref, cm.slots[s]
        npts = len(cloud)
        if ids is not None:
            mine = np.full(npts, -1, np.int32)
            mine[: min(npts, len(ids[i]))] = np.asarray(ids[i])[:npts]
            count = counts[i]
        else:
            mine, count = foreign_ids(ids_src, i, npts, M), foreign_count(cnt_src, i, M)
        cap = M if m != "box_cluster_count_unclamped" else box_ref.MAX_CLUSTERS
        p = ref._m.contents.position
        true_pos = (p[0], p[1])
        if m == "box_position_of_before_the_move" and sl.prev_pos is not None:
            p[0], p[1] = sl.prev_pos
        try:
            pos = (float(p[0]), float(p[1]))

            def compute():
                Mi = min(max(count, 0), cap)
                inside = np.zeros(npts, bool)
                for q in np.nonzero((mine >= 0) & (mine < Mi))[0]:
                    ok, r, c = ref.get_index(float(cloud["x"][q]), float(cloud["y"][q]))
                    inside[q] = ok and 0 <= r < ref.rows and 0 <= c < ref.cols
                return box_ref.expected_boxes(cloud["x"], cloud["y"], mine, count, pos, ref.resolution, rot, criterion, cap, inside)

            Mi, records, costs = sm._memo(("boxes", cm.shape, K, criterion, cap, count, pos, sm._digest(cloud), sm._digest(mine)), compute)
        finally:
            p[0], p[1] = true_pos
        out[f"cloud {i} (slot {s}) boxes"] = records
        if op["costs"]:
            out[f"cloud {i} (slot {s}) costs"] = costs
        reg["_live"].append(bool((records[:, 0] >= 0).any()))
    return out


def _rollouts_model(cm, op, m, out, reg):
    from tests import seq_model as sm

    n, K, rows = op["n"], op["K"], cm.rows
    ins = {name: sp._planes_in(cm, op[name], n) for name in ("mask", "cost", "clear")}
    dsrc = op["dist"]
    if dsrc is None:
        ins["dist"] = None
    elif sp.is_chained(dsrc):
        at = dsrc["op"]
        if m == "rollouts_dist_of_two_calls_ago":   # (of the heading calls with as many headings and rows)
            made = cm.outs.get(at)
            like = [j for j in sorted(cm.outs) if j < at and made is not None and "dist" in cm.outs[j] and cm.outs[j]["_op"].get("K") == K
                    and cm.outs[j]["_op"]["op"] == "route_headings" and len(cm.outs[j]["dist"]) >= dsrc["row0"] + n]
            at = like[-2] if len(like) >= 2 else at
        ins["dist"] = sp._planes_in(cm, dict(dsrc, op=at), n)
    else:
        ins["dist"] = [sm._memo(("foreign dist", json.dumps(dsrc, sort_keys=True), i, K, rows), lambda i=i: dist_volume(dsrc, i, K, rows)) for i in range(n)]
    if any(isinstance(v, str) for v in ins.values()):
        return None
    starts = start_words(op)
    if m == "rollouts_starts_of_the_previous_call" and cm.late.get("starts"):
        prev = cm.late["starts"]
        starts = [[prev[i % len(prev)][0], prev[i % len(prev)][1], prev[i % len(prev)][2] % K] for i in range(n)]
    cm.late["starts"] = start_words(op)
    rot = rollouts_ref.rotations_of(K)
    frame = rollouts_ref.RELATIVE if op["relative"] else rollouts_ref.ABSOLUTE
    cost_max = op["cost_max"] if m != "rollouts_cost_unclamped" else 1000
    order = sp.order_of(op)
    for i in range(n):
        ti = 0 if m == "rollouts_table_of_map_0_for_all" else i
        table = sm._memo(("rollout table", json.dumps(op["table"], sort_keys=True), ti if op["table"]["pad"] else 0, K, rows), lambda: make_table(op["table"], ti, K, rows))
        start = list(starts[i])
        use_rot = rot
        if m == "rollouts_start_heading_ignored" and op["relative"]:
            use_rot = np.repeat(rot[:1], K, axis=0)
        mask = np.ascontiguousarray(ins["mask"][i], dtype=np.int32)
        c = ins["cost"][i] if ins["cost"] is not None else None
        d = ins["dist"][i] if ins["dist"] is not None else None
        cl = ins["clear"][i] if ins["clear"] is not None else None
        dg = sm._digest
        key = ("rollouts", _key(op, "cost_max"), cost_max, ti, tuple(start), dg(use_rot), dg(mask), dg(c) if c is not None else b"", dg(d) if d is not None else b"",
               dg(cl) if cl is not None else b"")
        records, best = sm._memo(key, lambda: rollouts_ref.score_one(table, start, K, frame, use_rot, mask, c, d, cl, cost_max, op["reach"], order))
        out[f"map {i} records"] = records.astype(np.int32)
        if op["best"]:
            out[f"map {i} best"] = best.astype(np.int32)
        reg["_live"].append(bool(best[0] != -1))
    return out


def _clearance_model(cm, op, m, out, reg):
    from tests import cloud_refs
    from tests import seq_model as sm

    n = op["n"]
    seeds = sp._planes_in(cm, op["seeds"], n)
    if isinstance(seeds, str):
        return None
    order = sp.order_of(op)
    for i in range(n):
        words = np.asarray(seeds[i])
        occupied = words < 0 if m == "clearance_planes_sign_inverted" else words >= 0
        key = ("clearance planes", op["nearest"], op["max_cells"], order, cm.shape, sm._digest(occupied))
        if op["nearest"]:
            dist2, nearest, distance, count = sm._memo(key, lambda: clearance_ref.expected_clearance(occupied, op["max_cells"], order, cm.sh["res"]))
        else:
            dist2, distance, count = sm._memo(key, lambda: cloud_refs.expected_clearance_fast(occupied, op["max_cells"], cm.sh["res"]))
        out[f"map {i} dist2"] = dist2
        reg.setdefault("dist2", []).append(dist2)
        if op["nearest"]:
            out[f"map {i} nearest"] = nearest
        if op["distance"]:
            out[f"map {i} distance bits"] = distance
        if op["count"]:
            out[f"map {i} occupied cells"] = np.int32(count)
        reg["_live"].append(bool(count > 0))
    return out


def model_op(cm, op, m):
    """what the library must return for an op of LATE_KINDS: tests/box_ref.py, tests/rollouts_ref.py and tests/clearance_ref.py on the model's
    own copy of the chained buffers, and for the boxes the slot's position as the oracle map has it"""
    from tests import seq_model as sm

    if "expect" in op:
        return {"error": op["expect"], "nothing written": 1}
    if not hasattr(cm, "late"):
        cm.late = {}
    out = _base()
    if m == "plane_call_computes_lazy_layers" and any(cm.pred.state["lazy-owed"][s] for s in sm.touched(op, cm.n)):
        out["lazy maps kept"] = 0
    reg = {"_op": op, "_live": []}
    res = {"box_clusters": _box_model, "score_rollouts": _rollouts_model, "clearance_planes": _clearance_model}[op["op"]](cm, op, m, out, reg)
    if res is None:
        return {"undefined": 1}
    cm.outs[cm.at] = reg
    return res


# ---------------------------------------------------------------------------------------------------------------- the driver

def _input(d, op, src, n, ins, per_map=1):
    """(address, stride in words) of an input plane on the device: the earlier op's buffer where it stands, or seeded planes uploaded on the
    op's stream with `in_pad` junk words behind each.  An uploaded input is remembered in `ins` with its host copy: it is compared again
    at the checkpoint"""
    cells = d.seg.rows * d.seg.cols
    if src is None:
        return None, 0
    if sp.is_chained(src):
        t, stride, have, row_major = d.dev_outs[src["op"]][src["out"]][:4]
        assert row_major == op["row_major"] and have >= src["row0"] + n, "a chained plane keeps its order"
        return t.data_ptr() + 4 * src["row0"] * stride, stride
    stride = cells + int(op["in_pad"])
    host = np.full((n, stride), sp.JUNK, dtype=np.int32)
    for i in range(n):
        host[i, :cells] = sp.foreign_plane(src, i, d.seg.rows).ravel(order="C" if op["row_major"] else "F")
    dev = d._upload(host)
    ins.append((dev, host))
    return dev.data_ptr(), stride


def _up(d, host, ins):
    dev = d._upload(np.ascontiguousarray(host))
    ins.append((dev, np.ascontiguousarray(host)))
    return dev


def _box_points(d, op, x, ins):
    """the eight leading members of gg_cluster_boxes: the points of the batch or of the cluster call the op is chained to, where they lie;
    foreign clouds of its own uploaded on the op's stream.  Returns (n_points, cloud_stride, what must stay referenced)"""
    import ctypes as C

    from groundgrid_amd import _lib, api

    src, n = op["source"], op["n"]
    if src["mode"] == "chained":
        pts, _, n_pts, tfs = d.batches[src["batch"] if src.get("full") else d.mid[src["batch"]]]
        rec, stride, row0 = int(pts.shape[2]), int(pts.shape[1]), src["row0"]
        ptr, n_pts = pts.data_ptr() + row0 * stride * rec, n_pts[row0: row0 + n]
        tfs = None if tfs is None else tfs[row0: row0 + n]
    elif sp.is_chained(op["point_cluster"]):
        have = d.dev_outs[op["point_cluster"]["op"]]["_points"]
        ptr, stride, n_pts, rec, tfs = have["ptr"], have["stride"], have["n_points"][:n], have["rec"], have["tfs"]
    else:
        rec, stride = src["fmt"], src["stride"]
        clouds = [d.cloud(c) for c in src["clouds"]]
        n_pts = [len(c) for c in clouds]
        raw = np.zeros((n, stride, rec), dtype=np.uint8)
        for i, c in enumerate(clouds):
            raw[i, : len(c)] = np.frombuffer((api.pack16(c) if rec == 16 else c).tobytes(), dtype=np.uint8).reshape(-1, rec)
        ptr = _up(d, raw, ins).data_ptr()
        tfs = None if not src["tfs"] else np.stack([api.transform_from_pose(p, "kdl") for p in src["tfs"]])
    keep = [(C.c_int32 * n)(*op["slots"]), (C.c_int32 * n)(*[int(v) for v in n_pts])]
    x.n, x.first_slot, x.slots = n, (0 if op["slot_list"] else op["slots"][0]), (keep[0] if op["slot_list"] else None)
    x.point_format, x.d_points, x.cloud_stride, x.n_points = (_lib.GG_POINT16 if rec == 16 else _lib.GG_POINT32), ptr, stride, keep[1]
    if tfs is not None:
        keep.append(np.ascontiguousarray(np.asarray(tfs, dtype=np.float64).reshape(-1, 12)[:n]))
        x.transforms = keep[-1].ctypes.data_as(C.POINTER(C.c_double))
    return [int(v) for v in n_pts], stride, keep


def device_op(d, op):
    """the C call of an op of LATE_KINDS on its stream: sentinel-filled destinations with slack words and padded strides, a sentinel-filled
    twin where a nullable output is left out; nothing is downloaded before the checkpoint, where every word is compared -- the records at and
    beyond M_i, the words between 8 * P and the record stride, the twins, and the uploaded inputs as they were"""
    import ctypes as C

    from groundgrid_amd import _lib, api
    from tests import seq_model as sm

    kind, n, rows = op["op"], op["n"], d.seg.rows
    cells, L, ctx = rows * d.seg.cols, d.seg._L, d.seg._ctx
    keep, ins, bufs, reg = [], [], {}, {}
    order = None if kind == "box_clusters" else _lib.GG_PLANES_ROWMAJOR if op["row_major"] else _lib.GG_PLANES_COLMAJOR

    def dest(name, words):
        bufs[name] = d._words(words)
        return bufs[name].data_ptr()

    with d.on(op["stream"]):
        if kind == "box_clusters":
            x, fn = _lib.GGClusterBoxes(), L.gg_box_clusters
            n_pts, cstride, held = _box_points(d, op, x, ins)
            keep.append(held)
            M, K = op["M"], op["K"]
            if sp.is_chained(op["point_cluster"]):
                t, stride, have, _ = d.dev_outs[op["point_cluster"]["op"]]["point ids"]
                assert stride == cstride and have >= n
                x.d_point_cluster = t.data_ptr()
                x.d_n_clusters = d.dev_outs[op["n_clusters"]["op"]]["clusters"][0].data_ptr()
            else:
                ids = np.full((n, cstride), 0, dtype=np.int32)   # (behind a cloud's end: id 0, for a kernel that reads too far)
                for i in range(n):
                    ids[i, : n_pts[i]] = foreign_ids(op["point_cluster"], i, n_pts[i], M)
                x.d_point_cluster = _up(d, ids, ins).data_ptr()
                x.d_n_clusters = _up(d, np.array([foreign_count(op["n_clusters"], i, M) for i in range(n)], np.int32), ins).data_ptr()
            rot = np.ascontiguousarray(api.rotation_table(box_angles(K)), dtype=np.int32)
            keep.append(rot)
            x.rotations, x.n_rotations = rot.ctypes.data_as(C.POINTER(C.c_int32)), K
            x.criterion, x.max_clusters = (_lib.GG_BOX_EDGE if op["criterion"] == "edge" else _lib.GG_BOX_AREA), M
            x.d_boxes = dest("boxes", n * M * 8)
            costs = dest("costs", 2 * n * M * K + 1)   # (a twin when d_costs is left out)
            x.d_costs = (costs + 7) // 8 * 8 if op["costs"] else None
        elif kind == "score_rollouts":
            x, fn = _lib.GGRollouts(), L.gg_score_rollouts
            K, P, T = op["K"], op["table"]["P"], op["table"]["T"]
            x.n = n
            x.d_mask, x.mask_stride = _input(d, op, op["mask"], n, ins)
            x.d_cost, x.cost_stride = _input(d, op, op["cost"], n, ins)
            x.d_clear, x.clear_stride = _input(d, op, op["clear"], n, ins)
            if sp.is_chained(op["dist"]):   # the producer's volume as it stands, with its two strides
                t, dstride, have, row_major, pstride, k_made = d.dev_outs[op["dist"]["op"]]["dist"]
                assert row_major == op["row_major"] and k_made == K and have >= op["dist"]["row0"] + n
                x.d_dist, x.dist_stride, x.plane_stride = t.data_ptr() + 4 * op["dist"]["row0"] * dstride, dstride, pstride
            elif op["dist"] is not None:
                pstride = cells + int(op["in_pad"])
                host = np.full((n, K * pstride + 1), sp.JUNK, dtype=np.int32)
                for i in range(n):
                    vol = dist_volume(op["dist"], i, K, rows)
                    for k in range(K):
                        host[i, k * pstride: k * pstride + cells] = vol[k].ravel(order="C" if op["row_major"] else "F")
                x.d_dist, x.dist_stride, x.plane_stride = _up(d, host, ins).data_ptr(), K * pstride + 1, pstride
            x.n_headings = K
            x.starts = sp._host_i32(start_words(op), keep)
            if op["relative"]:
                x.rotations = sp._host_i32(api.rotation_table([2.0 * np.pi * k / K for k in range(K)]), keep)
            x.frame = _lib.GG_ROLLOUTS_RELATIVE if op["relative"] else _lib.GG_ROLLOUTS_ABSOLUTE
            tpad = int(op["table"]["pad"])
            tstride = 4 * P * T + tpad
            host = np.full((n if tpad else 1, tstride), sp.JUNK, dtype=np.int32)
            for i in range(len(host)):
                host[i, : 4 * P * T] = make_table(op["table"], i, K, rows).ravel()
            x.d_table, x.table_stride = _up(d, host, ins).data_ptr(), tstride if tpad else 0
            x.n_rollouts, x.n_steps, x.cost_max, x.reach, x.order = P, T, op["cost_max"], op["reach"], order
            rstride = 8 * P + int(op["pad"])
            x.d_records, x.record_stride = dest("records", n * rstride), rstride
            best = dest("best", n * 4)   # (a twin when d_best is left out)
            x.d_best = best if op["best"] else None
        else:
            x, fn = _lib.GGCloudClearance(), L.gg_clearance_clouds
            stride = cells + int(op["pad"])
            x.n = n
            x.d_seeds, x.seed_stride = _input(d, op, op["seeds"], n, ins)
            x.max_cells, x.order, x.plane_stride = op["max_cells"], order, stride
            if op.get("buf") is not None and "expect" not in op:   # a buffer that outlives checkpoints: filled when it is first used and never again
                key = ("late dist2", op["buf"], n, stride)
                if key not in d.chain_bufs:
                    d.chain_bufs[key] = d._words(n * stride)
                bufs["dist2"] = d.chain_bufs[key]
                x.d_dist2 = bufs["dist2"].data_ptr()
            else:
                x.d_dist2 = dest("dist2", n * stride)
            x.d_nearest = dest("nearest", n * stride) if op["nearest"] else None
            x.d_distance = dest("distance", n * stride) if op["distance"] else None
            x.d_n_occupied = dest("count", n) if op["count"] else None
            reg["dist2"] = (bufs["dist2"], stride, n, op["row_major"])
        if "expect" in op:   # an argument error: nothing is enqueued, nothing written, no ring entry taken
            if op["stream"] == "ctx":
                d.torch.cuda.current_stream(d.seg.device).synchronize()
            else:
                d.used.add(op["stream"])
            rc = fn(ctx, C.byref(x), d._stream_arg(op["stream"]))
            marks = None
        else:
            marks = d._enqueue(op, lambda st: fn(ctx, C.byref(x), st))
    d.keep.append((bufs, keep, ins))
    if "expect" not in op:
        d.dev_outs[d.at] = reg

    def collect():
        host = {name: t.cpu().numpy() for name, t in bufs.items()}
        untouched = lambda a: bool(np.all(a.view(np.uint32) == sm.SENTINEL))   # noqa: E731
        if "expect" in op:
            return {"error": _lib.STATUS.get(rc, rc), "nothing written": int(all(untouched(a) for a in host.values()))}
        res = d._marks_kept(marks)
        clean = True
        if kind == "box_clusters":
            M, K = op["M"], op["K"]
            counts = d.dev_outs[op["n_clusters"]["op"]]["clusters"][0].cpu().numpy() if sp.is_chained(op["n_clusters"]) else \
                np.array([foreign_count(op["n_clusters"], i, M) for i in range(n)])
            boxes = host["boxes"]
            clean &= untouched(boxes[n * M * 8:])
            skip = ((costs + 7) // 8 * 8 - costs) // 4   # (words in front of the 8-byte boundary)
            cw = host["costs"]
            if not op["costs"]:
                clean &= untouched(cw)
            else:
                clean &= untouched(cw[:skip]) and untouched(cw[skip + 2 * n * M * K:])
            for i, s in enumerate(op["slots"]):
                Mi = min(max(int(counts[i]), 0), M)
                row = boxes[i * M * 8: (i + 1) * M * 8]
                res[f"cloud {i} (slot {s}) boxes"] = row[: Mi * 8].reshape(-1, 8)
                clean &= untouched(row[Mi * 8:])
                if op["costs"]:
                    crow = cw[skip + 2 * i * M * K: skip + 2 * (i + 1) * M * K]
                    res[f"cloud {i} (slot {s}) costs"] = np.ascontiguousarray(crow[: 2 * Mi * K]).view(np.uint64).reshape(-1, K)
                    clean &= untouched(crow[2 * Mi * K:])
        elif kind == "score_rollouts":
            P = op["table"]["P"]
            rstride = 8 * P + int(op["pad"])
            a = host["records"]
            clean &= untouched(a[n * rstride:])
            for i in range(n):
                row = a[i * rstride: (i + 1) * rstride]
                res[f"map {i} records"] = row[: 8 * P].reshape(P, 8)
                clean &= untouched(row[8 * P:])
            if op["best"]:
                clean &= untouched(host["best"][4 * n:])
                for i in range(n):
                    res[f"map {i} best"] = host["best"][4 * i: 4 * i + 4]
            else:
                clean &= untouched(host["best"])
        else:
            stride = cells + int(op["pad"])
            for name, key in (("dist2", "dist2"), ("nearest", "nearest"), ("distance", "distance bits")):
                if name in host:
                    planes, ok = d._planes(host[name], n, 1, stride, op["row_major"])
                    clean &= ok
                    for i, p in enumerate(planes):
                        res[f"map {i} {key}"] = p.view(np.uint32) if name == "distance" else p
            if "count" in host:
                clean &= untouched(host["count"][n:])
                for i in range(n):
                    res[f"map {i} occupied cells"] = np.int32(host["count"][i])
        res["nothing else written"] = int(clean)
        res["inputs as they were"] = int(all(np.array_equal(dev.cpu().numpy(), was) for dev, was in ins))
        return res

    return collect
